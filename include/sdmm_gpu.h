/*
 * sdmm_gpu.h -- C ABI of the MI355X-native SDMM path-guiding hot path.
 *
 * This is the drop-in boundary the Mitsuba `sdmm` integrator plugin calls in
 * place of the (absent) sdmm-lib submodule.  Every entry point names the
 * reference interface it replaces (paths relative to anadodik/sdmm-mitsuba):
 *
 *   sdmm_create / sdmm_destroy    SDMMContext construction
 *                                 (mitsuba/src/integrators/sdmm/sdmm_proc.h:92-93)
 *   sdmm_init_hemisphere          sdmm::initialize  (volpath_sdmm.cpp:132-138);
 *                                 math: jmm uniformHemisphereInit
 *                                 (dmm/jmm/mixture_model_init.h:79-242)
 *   sdmm_em_step                  sdmm::em_step     (volpath_sdmm.cpp:220, :304)
 *                                 + sdmm::prepare   (volpath_sdmm.cpp:237, :307);
 *                                 math: jmm StepwiseTangentEM::optimize
 *                                 (dmm/jmm/opt/stepwise_tangent.h:597-1053)
 *   sdmm_em_step_batched          the plugin's per-leaf optimisation loop: one
 *                                 sdmm::em_step per tree leaf, run on a thread
 *                                 pool (volpath_sdmm.cpp:244-312, leaf filter
 *                                 :140-149), as ONE batched device launch
 *   sdmm_estep_stats/sdmm_mstep   the same EM step split around the
 *                                 sufficient-statistics all-reduce (multi-GPU)
 *   sdmm_responsibilities         MixtureModel::posteriorAndLog over a batch
 *                                 (dmm/jmm/mixture_model.h:146-192)
 *   sdmm_guide_batch              sdmm::create_conditional + conditional.sample
 *                                 + posterior/hsum_nested (sdmm_proc.cpp:368,
 *                                 :411-421, :539-545); math: jmm
 *                                 MixtureModel::conditional/sample/pdf
 *                                 (mixture_model.h:235-304, :72-75, :113-121)
 *   sdmm_pdf_batch                pdfSurface's gmmPdf (sdmm_proc.cpp:510-590)
 *   sdmm_get_params/set_params    sdmm::save_json / load_json
 *                                 (volpath_sdmm.cpp:121-130; bsdfs/diffuse.cpp:101-114)
 *
 * Conventions: plain C types only; every function returns SDMM_OK (0) or a
 * negative SDMM_E* code and sets a thread-local message (sdmm_last_error).
 * No C++ exception crosses the ABI.  Pointers documented "device" must be
 * HBM-resident allocations on the handle's device; "host" pointers are
 * ordinary memory, read-only during the call.  A handle is re-entrant
 * against other handles; calls on one handle must be serialised by the
 * caller.  Work is enqueued on the handle's HIP stream (sdmm_set_stream);
 * functions that return data to host memory synchronise that stream.
 * Host threads may call the library at once on distinct handles (the
 * reference's per-leaf worker threads, volpath_sdmm.cpp:287-311, and render
 * threads, sdmm_proc.cpp:1086-1106): host data moves through the calling
 * thread's pinned bounce buffer (never a DMA from caller memory), per-call
 * device scratch is pooled per (device, stream), and no buffer is freed
 * before the stream that used it has been synchronised.
 */
#ifndef SDMM_GPU_H
#define SDMM_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDMM_ABI_VERSION 1

enum {
    SDMM_OK = 0,
    SDMM_E_INVALID = -1,   /* bad argument / unsupported K */
    SDMM_E_HIP = -2,       /* HIP runtime error */
    SDMM_E_STATE = -3,     /* handle not initialised */
    SDMM_E_NOMEM = -4
};

typedef struct sdmm_mix sdmm_mix;

/* StepwiseTangentEM constructor arguments (stepwise_tangent.h:221-252). */
typedef struct {
    float alpha;              /* 0.9   stepwise exponent */
    float bprior[5];          /* 1e-5  diagonal covariance prior (overwritten by init) */
    float ni_prior_minus_one; /* 6e-5  weight prior */
    double epsilon;           /* 1e-100 depth-prior diagonal (as float: 0) */
    int decrease_prior;       /* 1 */
} sdmm_em_params;

/* SoA sample batch, one plane per field (Samples<6,float>, samples.h:32-46). */
typedef struct {
    const float* x[6];          /* normalised position (3) + unit direction (3) */
    const float* w;             /* weight */
    const float* hpdf;          /* heuristic pdf, may be NULL */
    const uint8_t* is_diffuse;  /* heuristic flag, may be NULL */
    int64_t n;
} sdmm_samples;

/* Fill p with the reference defaults. */
void sdmm_em_params_default(sdmm_em_params* p);

/* Create a K-component mixture (1 <= K <= 512) on HIP device `device`. */
int sdmm_create(int K, const sdmm_em_params* params, int device, sdmm_mix** out);
/* Stream-ordered creation: the allocation (hipMallocAsync) and initialisation
 * are enqueued on hip_stream, which the handle then uses; nothing waits on the
 * host.  For the many small per-leaf mixtures of a guiding tree.  The stream
 * must outlive the handle (its memory is freed on it). */
int sdmm_create_on_stream(int K, const sdmm_em_params* params, int device, void* hip_stream, sdmm_mix** out);
/* n such handles from ONE stream-ordered slab (one allocation, one
 * initialisation launch for all); the slab is freed with its last handle. */
int sdmm_create_many_on_stream(int K, const sdmm_em_params* params, int device, void* hip_stream, int n,
                               sdmm_mix** out);
void sdmm_destroy(sdmm_mix* m);
int sdmm_num_components(const sdmm_mix* m);
/* Diagnostics: E-step kernel layouts (components per lane, lanes per sample)
 * of the responsibility and statistics kernels.  Any pointer may be NULL. */
int sdmm_layout(const sdmm_mix* m, int* resp_cpl, int* resp_lps, int* stats_cpl, int* stats_lps);
/* Diagnostics: name of the kernel the handle launches for the responsibility
 * (which = 0) or statistics (which = 1) E-step; "" for a NULL handle. */
const char* sdmm_kernel_name(const sdmm_mix* m, int which);
/* Diagnostics: how many times the handle has built the coefficient image of
 * its responsibility kernel (estep_resp_split_kernel reads one image per
 * mixture; it is rebuilt by the first sdmm_responsibilities after a change of
 * the parameters, not per call).  0 for handles that use another kernel or
 * run with SDMM_RESP_IMAGE=inline. */
int sdmm_resp_image_builds(const sdmm_mix* m, int64_t* count);
/* Guided queries keep a per-query list of at most `cap` candidate components
 * (default 40, maximum 64); queries that do not fit take the full-K path.
 * Results are identical for every cap; 0 sends every query down the full-K
 * path (a testing knob).  A tree wavefront uses the smallest cap of the
 * mixtures bound to it (read when the table is bound / passed). */
int sdmm_set_guide_capacity(sdmm_mix* m, int cap);
/* coherent != 0 (default): guided batches of >= 16384 queries are served in
 * Morton order of their condition position (a device radix sort of the
 * batch), so the queries of a wave touch the same components.  Outputs are
 * written at each query's own index and are identical either way. */
int sdmm_set_guide_order(sdmm_mix* m, int coherent);
/* Diagnostics: how many queries of the handle's last guided call (guide, pdf,
 * product) took the full-K fallback path.  Synchronises the handle's stream. */
int sdmm_guide_fallback_count(const sdmm_mix* m, int* count);
/* Work is enqueued on this hipStream_t, taken literally (NULL = the HIP null
 * stream).  A new handle starts on its own non-blocking stream, whose value
 * sdmm_get_stream returns before any sdmm_set_stream call. */
int sdmm_set_stream(sdmm_mix* m, void* hip_stream);
void* sdmm_get_stream(const sdmm_mix* m);
int sdmm_synchronize(sdmm_mix* m);

/* uniformHemisphereInit with given seed positions/normals (host, n_pos*3 each);
 * K must equal 8 * n_pos.  depth_prior / min_spatial_distance in normalised
 * scene units; seed drives the PCG32 direction jitter. */
int sdmm_init_hemisphere(sdmm_mix* m, const float* positions, const float* normals, int n_pos,
                         float depth_prior, float min_spatial_distance, uint64_t seed);

/* sdmm_init_hemisphere for n mixtures of one K at once (mixture i: K/8
 * positions / normals at positions + 3 (K/8) i, its own spatial distance and
 * seed): one host synchronisation for the whole set (the guiding model's new
 * leaves). */
int sdmm_init_hemisphere_batched(sdmm_mix* const* mixes, int n, const float* positions, const float* normals,
                                 float depth_prior, const float* min_spatial_distance, const uint64_t* seeds);

/* kMeansPPInit (dmm/jmm/mixture_model_init.h:244-330) on the device: for each
 * of n_leaves leaves -- samples [seg[l], seg[l+1]) of the device planes s->x[0..2]
 * (positions), normals[0..2] and s->w -- the k-means++ choice of n_pos seed
 * samples, draw i using uniforms[l * n_pos + i] (the rng() calls, in order).
 * out_index (host, n_leaves * n_pos): leaf-relative sample indices;
 * out_positions / out_normals (host, 3 per draw, may be NULL): the chosen
 * samples' positions and normals.  Weights
 * and their sums in fp64 (the reference forms a float CDF; the choice differs
 * only where a draw falls within its rounding of a boundary).  One workgroup
 * per leaf on hip_stream; returns after the indices are on the host. */
int sdmm_kmeanspp_select(const sdmm_samples* s, const float* const normals[3], const int64_t* seg, int n_leaves,
                         int n_pos, const float* uniforms, int device, void* hip_stream, int64_t* out_index,
                         float* out_positions, float* out_normals);

/* uniformHemisphereInit with kMeansPlusPlus = true (:130-138) for n mixtures
 * of one K: mixture i's K/8 positions / normals chosen by sdmm_kmeanspp_select
 * over samples [seg[i], seg[i+1]); its PCG32 stream (seeds[i]) gives the
 * K/8 k-means++ draws and then the direction jitter. */
int sdmm_init_hemisphere_kmeanspp_batched(sdmm_mix* const* mixes, int n, const sdmm_samples* s,
                                          const float* const normals[3], const int64_t* seg, float depth_prior,
                                          const float* min_spatial_distance, const uint64_t* seeds);

/* Host-only variant (no device, no handle): writes the initial component
 * parameters, for data generators and tests.  Arrays sized K=8*n_pos. */
int sdmm_hemisphere_init_host(const float* positions, const float* normals, int n_pos,
                              float depth_prior, float min_spatial_distance, uint64_t seed,
                              float* weights /*K*/, float* means /*K*6*/, float* covs /*K*25*/,
                              float* bpriors /*K*25*/, float* bdepth /*K*9*/);

/* One stepwise EM iteration (`iterations` times) over device-resident samples. */
int sdmm_em_step(sdmm_mix* m, const sdmm_samples* device_samples, int iterations);
/* Same with host-resident samples (staged through the handle's buffers). */
int sdmm_em_step_host(sdmm_mix* m, const sdmm_samples* host_samples, int iterations);

/* Batched per-leaf EM (the spatial tree's leaves, each its own mixture):
 * mixes[i] takes one stepwise EM iteration (`iterations` times) over samples
 * [seg[i], seg[i+1]) of the device planes `device_samples` (the leaves' data
 * stored back to back).  seg: host, n_mix + 1 non-decreasing offsets within
 * [0, device_samples->n]; a leaf with no samples is left unchanged (like
 * sdmm_em_step with n = 0).  All handles must share K and the device and be
 * distinct; the work runs on mixes[0]'s stream (the other handles' streams
 * are synchronised on entry and wait for the batch on exit).  Results are
 * bitwise those of sdmm_em_step(mixes[i], leaf i) called one by one. */
int sdmm_em_step_batched(sdmm_mix* const* mixes, int n_mix, const sdmm_samples* device_samples,
                         const int64_t* seg, int iterations);
/* Per-leaf iteration counts (the built plugin's optimize(): 2 EM iterations
 * for a leaf while its em.iterations_run < 4, else 1, volpath_sdmm.cpp:299-305):
 * round t steps every leaf with iterations[i] > t; bitwise the same as
 * sdmm_em_step(mixes[i], leaf i, iterations[i]) one by one. */
int sdmm_em_step_batched_iters(sdmm_mix* const* mixes, int n_mix, const sdmm_samples* device_samples,
                               const int64_t* seg, const int* iterations);
/* Same with host-resident planes (staged through mixes[0]'s buffers; returns
 * after the batch, so the host planes may be reused). */
int sdmm_em_step_batched_host(sdmm_mix* const* mixes, int n_mix, const sdmm_samples* host_samples,
                              const int64_t* seg, int iterations);
int sdmm_em_step_batched_host_iters(sdmm_mix* const* mixes, int n_mix, const sdmm_samples* host_samples,
                                    const int64_t* seg, const int* iterations);

/* Split-phase EM step for sample-sharded multi-GPU runs:
 *   sdmm_estep_stats  writes this shard's fp64 sufficient statistics,
 *                     layout [H, weightSum, W(K), M(5K), C_lower(15K)],
 *                     sdmm_stats_len(K) doubles, into `stats` (device);
 *   (caller all-reduces `stats` with a SUM over ranks, e.g. ncclAllReduce)
 *   sdmm_mstep        consumes the global statistics; n_total = global sample
 *                     count (samples.size() of the reference), >= 0
 *                     (SDMM_E_INVALID otherwise).                           */
size_t sdmm_stats_len(int K);
int sdmm_estep_stats(sdmm_mix* m, const sdmm_samples* device_samples, double* stats);
int sdmm_mstep(sdmm_mix* m, const double* stats, int64_t n_total);

/* Multi-GPU.  One process per GPU; a communicator joins the ranks
 * that train the same mixtures.  Transports:
 *   RCCL   sdmm_comm_unique_id on one rank, the 128 bytes shared by the caller
 *          (MPI, a file, torch.distributed), then sdmm_comm_init_rccl on every
 *          rank (collectives on the mixtures' HIP streams, over xGMI);
 *   host   sdmm_comm_init_host with the caller's own collective on HOST buffers
 *          (allreduce: in-place SUM of count doubles; broadcast: in-place from
 *          rank root); the library stages through pinned memory.  Callbacks
 *          return 0 on success.
 * Every rank must make the same sequence of sharded calls.
 *   sdmm_em_step_sharded   sample-sharded StepwiseTangentEM::optimize
 *                          (stepwise_tangent.h:597-1053): this rank's shard's
 *                          statistics, ONE all-reduce (sum) of [H, wsum, W, M,
 *                          Clow, n] fp64, then the same M-step on every rank
 *                          (identical parameters everywhere, no broadcast).
 *                          The reference's own sharded-statistics pattern is the
 *                          legacy jmm/opt/stepwise.h:248-396 (threads + mutex).
 *   sdmm_em_step_batched_sharded  the per-leaf EM with every rank holding
 *                          samples of every leaf: the batched statistics of all
 *                          leaves (+ counts) in ONE all-reduce per iteration
 *                          round, then the batched M-step on every rank.
 *   sdmm_mix_broadcast     leaf-sharded EM: after each rank stepped the leaves it
 *                          owns (owner[i] == rank, e.g. sdmm_em_step_batched on
 *                          that subset), every leaf's parameters and stepwise
 *                          state are broadcast from its owner (RCCL: one fused
 *                          group), so all ranks hold all leaves for guiding. */
typedef struct sdmm_comm sdmm_comm;
#define SDMM_COMM_ID_BYTES 128
typedef int (*sdmm_host_allreduce_f64)(double* buf, size_t count, void* user);
typedef int (*sdmm_host_broadcast)(void* buf, size_t bytes, int root, void* user);
int sdmm_comm_unique_id(void* id /* SDMM_COMM_ID_BYTES */);
int sdmm_comm_init_rccl(const void* id, int nranks, int rank, int device, sdmm_comm** out);
int sdmm_comm_init_host(int nranks, int rank, int device, sdmm_host_allreduce_f64 allreduce,
                        sdmm_host_broadcast broadcast, void* user, sdmm_comm** out);
void sdmm_comm_destroy(sdmm_comm* c);
int sdmm_comm_rank(const sdmm_comm* c);
int sdmm_comm_size(const sdmm_comm* c);
/* in-place SUM of count device doubles over the ranks, on hip_stream */
int sdmm_comm_allreduce_f64(sdmm_comm* c, double* buf, size_t count, void* hip_stream);
int sdmm_em_step_sharded(sdmm_mix* m, sdmm_comm* c, const sdmm_samples* device_shard, int iterations);
int sdmm_em_step_batched_sharded(sdmm_mix* const* mixes, int n_mix, sdmm_comm* c, const sdmm_samples* device_samples,
                                 const int64_t* seg, const int* iterations);
int sdmm_mix_broadcast(sdmm_mix* const* mixes, int n_mix, const int32_t* owner, sdmm_comm* c);

/* Posterior (responsibility) of every sample: resp[n*K + k], device, fp32. */
int sdmm_responsibilities(sdmm_mix* m, const sdmm_samples* device_samples, float* resp);

/* Guided bounce for nq queries (device SoA planes):
 *   c[3]   normalised condition position     u[3]  uniforms (cdf, Box-Muller)
 *   d[3]   sampled world direction (out)     pdf   conditional mixture pdf at d
 *   comp   joint component index used (-1: no valid conditional -> BSDF only) */
int sdmm_guide_batch(const sdmm_mix* m, int64_t nq, const float* const c[3], const float* const u[3],
                     float* const d[3], float* pdf, int32_t* comp);
/* gmmPdf of given directions d (device SoA). */
int sdmm_pdf_batch(const sdmm_mix* m, int64_t nq, const float* const c[3], const float* const d[3],
                   float* pdf);
/* Product sampling with a learned BSDF -- sampleSurface / pdfSurface with
 * sampleProduct (sdmm_proc.cpp:327-392, :474-486): the query's conditional
 * times the learned-BSDF lobes of its material (sdmm::product, absent;
 * restated from jmm MixtureModel::multiply, mixture_model.h:345-370, and
 * MVTN::multiply, multivariate_tangent_normal.h:555-617), then sample / pdf
 * of the product.  Device arrays:
 *   bsdf      B materials x M (<= 64) directional lobes in the LOCAL shading
 *             frame, already oriented for wi (sdmm-lib's rotate_to_wo is the
 *             caller's): weights [B][M], unit means [B][M][3], 2x2 covariances
 *             [B][M][4] in each lobe's tangent frame Coordinates(mean)
 *   material  per query; < 0 (or >= B): no learned BSDF
 *   frame[9]  per-query to-world matrix F, row-major, columns s, t, n
 *             (sdmm_proc.cpp:348-352); lobes go to world as mean F m,
 *             frame to F^T (:353-356)
 *   heuristic (nullable) per query heuristicConditionalWeight (:383-392):
 *             0.3 product, 0.5 plain conditional (no BSDF / empty product),
 *             1 no valid conditional (BSDF only)
 * comp = k * M + j (joint component k, lobe j) for product samples, the
 * joint index for plain-conditional samples, -1 for BSDF only.  Bit-exact
 * against oracle/sdmm_oracle_product.inc in comp; pdf of given directions
 * d with sdmm_pdf_product_batch. */
typedef struct {
    const float* weights;
    const float* means;
    const float* covs;
    int B, M;
    /* per material (nullable): 1 = a diffuse BSDF.  The plugin's diffuse case
     * (sdmm_proc.cpp:335-339) re-centres only slice 0 on the shading normal
     * (set_mean(normal): mean = F's third column, frame Coordinates(mean));
     * slices >= 1 are then used as stored, in world coordinates. */
    const uint8_t* diffuse;
} sdmm_bsdf_table;
int sdmm_guide_product_batch(const sdmm_mix* m, int64_t nq, const float* const c[3], const float* const u[3],
                             const sdmm_bsdf_table* bsdf, const int32_t* material, const float* const frame[9],
                             float* const d[3], float* pdf, int32_t* comp, float* heuristic);
int sdmm_pdf_product_batch(const sdmm_mix* m, int64_t nq, const float* const c[3], const float* const d[3],
                           const sdmm_bsdf_table* bsdf, const int32_t* material, const float* const frame[9],
                           float* pdf, float* heuristic);
/* lower_bound + tie walk of utils.h:104-115 on a caller CDF (device). */
int sdmm_sample_discrete_cdf(const sdmm_mix* m, const float* cdf, int n, const float* u, int64_t nq,
                             int32_t* out);

/* Export the mixture (host outputs, any may be NULL): the canonical MVTN
 * parameters plus every derived array, in the oracle's or_mixture layout. */
typedef struct {
    float* weights;    /* K */
    float* cdf;        /* K */
    float* mean;       /* K*6 */
    float* cov;        /* K*25 */
    float* to;         /* K*9 */
    float* cholL;      /* K*25 */
    float* cholLInv;   /* K*25 */
    float* detInv;     /* K */
    float* muPremult;  /* K*6 */
    float* condCov;    /* K*4 */
    float* margL;      /* K*9 */
    float* margDetInv; /* K */
    float* condL;      /* K*4 */
    float* condLInv;   /* K*4 */
    float* condDetInv; /* K */
    int32_t* valid;    /* K */
    float* normalization; /* 1 */
} sdmm_params_out;
int sdmm_get_params(const sdmm_mix* m, const sdmm_params_out* out);
/* Replace the mixture by (weights, means, covs) host arrays; runs MVTN::set. */
int sdmm_set_params(sdmm_mix* m, const float* weights, const float* means, const float* covs);

/* Stepwise state export/import (checkpointing, tests).  Host buffers:
 * scalars[9] = {heuristicTotalWeight, sgH, normalization, iterationsRun,
 * alpha, niPriorMinusOne, decreasePrior, trainingCutoff, lastStatus};
 * T[K], sgW[K], sgM[5K], sgC[25K] (double); bpriors[25K], bdepth[9K] (float). */
/* iterations_run of n mixtures (StepwiseTangentEM::iterationsRun, the
 * plugin's 2-while-below-4 schedule, volpath_sdmm.cpp:299-302), one wait. */
int sdmm_iterations_run(const sdmm_mix* const* mixes, int n, int* out);
int sdmm_get_state(const sdmm_mix* m, double* scalars, double* T, double* sgW, double* sgM,
                   double* sgC, float* bpriors, float* bdepth);
int sdmm_set_state(sdmm_mix* m, const double* scalars, const double* T, const double* sgW,
                   const double* sgM, const double* sgC, const float* bpriors, const float* bdepth);

/* Spatial tree (the plugin's accelerator: sdmm-lib DMMSTree, sdmm_proc.h:91,
 * absent; restated from jmm SNTree, dmm/jmm/sntree.h:93-299, spatial part).
 * Node ids are the reference's m_nodes indices; child 0 is the upper part of
 * a split.  Construction is host work (as in the reference); find and route
 * run on the device, on the tree's own stream.
 *   sdmm_stree_create          root = the AABB enlarged to a cube (:101-106)
 *   sdmm_stree_split_to_depth  split_to_depth (:195-233); the built plugin
 *                              calls split_to_depth(2) (sdmm/volpath_sdmm.cpp:398)
 *   sdmm_stree_split           split(threshold) (:235-283) on HOST position
 *                              planes p[3] (n points): every leaf, no leaf cap
 *   sdmm_stree_find            STree.find(key) (sdmm_proc.cpp:314, :923, :954)
 *                              for n DEVICE points -> node id or -1 (outside);
 *                              depth first with backtracking (sntree.h:62-83)
 *   sdmm_stree_route           device samples -> device planes `out` (same n,
 *                              same optional planes) in leaf-contiguous order,
 *                              stable within a leaf; seg (host, num_nodes + 1):
 *                              node v's samples are [seg[v], seg[v+1]), points
 *                              outside the tree follow seg[num_nodes].  `seg`
 *                              with the leaves' mixtures feeds
 *                              sdmm_em_step_batched directly. Synchronous. */
typedef struct sdmm_stree sdmm_stree;
int sdmm_stree_create(const float aabb_min[3], const float aabb_max[3], int device, sdmm_stree** out);
void sdmm_stree_destroy(sdmm_stree* t);
int sdmm_stree_split_to_depth(sdmm_stree* t, int max_depth);
int sdmm_stree_split(sdmm_stree* t, const float* const p[3], int64_t n, int threshold);
int sdmm_stree_num_nodes(const sdmm_stree* t);
/* The built plugin's tree calls (sdmm/volpath_sdmm.cpp):
 *   sdmm_stree_leaf_nodes          m_accelerator->leaf_nodes() (:182, :253)
 *   sdmm_stree_split_leaf_recurse  split_leaf_recurse(node_i, threshold)
 *                                  (:184, :257): node's samples p (host planes,
 *                                  the node's stats positions); a leaf holding
 *                                  more than threshold is split and its children
 *                                  recursively; an inner node is left alone
 *   sdmm_stree_split_leaves        the whole splitting block of optimize() /
 *                                  optimize_async_run() (:181-186, :253-260):
 *                                  if leaf_nodes() <= max_leaf_nodes (2048,
 *                                  :529), split_leaf_recurse(i, threshold (4000,
 *                                  :528)) for every node, the samples routed to
 *                                  the leaves by find. */
int sdmm_stree_leaf_nodes(const sdmm_stree* t);
int sdmm_stree_split_leaf_recurse(sdmm_stree* t, int node, const float* const p[3], int64_t n, int threshold);
int sdmm_stree_split_leaves(sdmm_stree* t, const float* const p[3], int64_t n, int threshold, int max_leaf_nodes);
/* split_leaf_recurse for n nodes at once (increasing ids), node i with its
 * own counts[i] positions at planes p[3i..3i+2]: leaves split on parallel host
 * threads, the new nodes numbered exactly as n sequential calls would. */
int sdmm_stree_split_leaf_recurse_many(sdmm_stree* t, int n, const int32_t* nodes, const float* const* p,
                                       const int64_t* counts, int threshold);
/* The same on DEVICE-resident positions: node i's counts[i] positions are
 * entries [starts[i], starts[i] + counts[i]) of the device planes p[0..2].
 * The recursion runs on the device level by level (fp64 sums in the same
 * fixed order as the host split's, the per-node decisions on the host, a
 * stable partition per level); the node arrays are identical to
 * sdmm_stree_split_leaf_recurse_many's.  On the tree's stream; synchronous. */
int sdmm_stree_split_leaf_recurse_device(sdmm_stree* t, int n, const int32_t* nodes, const float* const p[3],
                                         const int64_t* starts, const int64_t* counts, int threshold);
/* aabb[6 * i] = min(3), max(3); child[2 * i] = children (-1, -1 for a leaf);
 * axis[i]: split axis.  Any output may be NULL. */
int sdmm_stree_get_nodes(const sdmm_stree* t, float* aabb, int32_t* child, int32_t* axis);
int sdmm_stree_find(sdmm_stree* t, int64_t n, const float* const p[3], int32_t* node_out);
int sdmm_stree_route(sdmm_stree* t, const sdmm_samples* device_samples, const sdmm_samples* out, int64_t* seg);
/* The tree's HIP stream, taken literally (NULL = the HIP null stream); before
 * any sdmm_stree_set_stream call the tree uses its own non-blocking stream.  A
 * wavefront waits (events) for pending work of the bound mixtures on their own
 * streams, so an EM step enqueued before it is complete when it reads the
 * mixtures; its outputs are ready once the tree's stream is. */
int sdmm_stree_set_stream(sdmm_stree* t, void* hip_stream);
void* sdmm_stree_get_stream(const sdmm_stree* t);

/* Guided wavefront over the tree's leaves -- SDMMRenderer::sampleSurface for
 * a batch of bounces (sdmm_proc.cpp:309-421): per query, node =
 * STree.find(c) (:314), that node's mixture node_mix[node] (host array of
 * sdmm_stree_num_nodes handles; NULL or uninitialised = no trained context,
 * and a query outside the tree: BSDF only, :316-323), then conditional /
 * sample / pdf exactly as sdmm_guide_batch against that mixture (outputs
 * bitwise equal to it; comp -1 and pdf 0 when there is no valid conditional).
 * node_out (nullable): node id per query (-1 outside).  Runs on the tree's
 * stream; the mixtures must have no pending work on other streams.
 * node_mix NULL: use the table bound by sdmm_stree_bind_mixtures (the
 * plugin binds once per training iteration, after the per-leaf EM; the
 * table re-uploads only when a handle/K changes).
 *   sdmm_pdf_wavefront   pdfSurface's gmmPdf of given directions d
 *                        (sdmm_proc.cpp:510-590) per query's own leaf. */
int sdmm_stree_bind_mixtures(sdmm_stree* t, const sdmm_mix* const* node_mix);
int sdmm_guide_wavefront(sdmm_stree* t, const sdmm_mix* const* node_mix, int64_t nq, const float* const c[3],
                         const float* const u[3], float* const d[3], float* pdf, int32_t* comp,
                         int32_t* node_out);
int sdmm_pdf_wavefront(sdmm_stree* t, const sdmm_mix* const* node_mix, int64_t nq, const float* const c[3],
                       const float* const d[3], float* pdf);
/* One guided bounce of a whole wavefront, sampleSurface + pdfSurface with the
 * plugin's BSDF/guide mixing (sdmm_proc.cpp:383-421, :474-502): the per-query
 * conditional is built ONCE; query q then either samples it (pdf_mode[q] == 0:
 * d, pdf, comp exactly as sdmm_guide_wavefront) or evaluates its gmmPdf at the
 * BSDF-sampled direction dgiven[q] (pdf_mode[q] != 0: pdf exactly as
 * sdmm_pdf_wavefront, d[q] = dgiven[q], comp[q] = -2 when the conditional is
 * valid, -1 when not -- the reference's validConditional, :368-392). */
int sdmm_guide_pdf_wavefront(sdmm_stree* t, const sdmm_mix* const* node_mix, int64_t nq, const float* const c[3],
                             const float* const u[3], const float* const dgiven[3], const uint8_t* pdf_mode,
                             float* const d[3], float* pdf, int32_t* comp, int32_t* node_out);

/* Product sampling over the spatial tree's leaves -- sampleSurface /
 * pdfSurface with sampleProduct for a wavefront of bounces (sdmm_proc.cpp:
 * 309-392, :474-502): per query, node = STree.find(c), that node's mixture
 * (node_mix or the table bound by sdmm_stree_bind_mixtures; none: BSDF only,
 * h = 1, comp -1, pdf 0), then exactly sdmm_guide_product_batch /
 * sdmm_pdf_product_batch against it (outputs bitwise equal).
 *   choice (nullable, device): the mixed bounce -- query q's BSDF/guide draw;
 *          with it, dgiven (device, 3 planes: the BSDF-sampled directions) is
 *          required and query q becomes a pdf query at dgiven[q] when
 *          choice[q] <= h[q] (the reference's rRec.nextSample1D() <=
 *          heuristicConditionalWeight, :392, with h 0.3 for a usable product,
 *          0.5 for the plain conditional): d = dgiven, pdf = the used
 *          mixture's pdf there, comp = -2.  Without choice, every query samples.
 *   heuristic (nullable): per query h (0.3 / 0.5 / 1); node_out (nullable). */
int sdmm_guide_product_wavefront(sdmm_stree* t, const sdmm_mix* const* node_mix, int64_t nq, const float* const c[3],
                                 const float* const u[3], const float* choice, const float* const dgiven[3],
                                 const sdmm_bsdf_table* bsdf, const int32_t* material, const float* const frame[9],
                                 float* const d[3], float* pdf, int32_t* comp, float* heuristic, int32_t* node_out);
int sdmm_pdf_product_wavefront(sdmm_stree* t, const sdmm_mix* const* node_mix, int64_t nq, const float* const c[3],
                               const float* const d[3], const sdmm_bsdf_table* bsdf, const int32_t* material,
                               const float* const frame[9], float* pdf, float* heuristic);

/* Concurrent guided bounces from many render threads -- the reference's
 * render workers call create_conditional / sample / pdf at once, each with
 * thread_local scratch (sdmm_proc.cpp:1086-1106, volpath_sdmm.cpp:411-507).
 *   sdmm_stree_publish   make the tree's current state readable from guide
 *                        contexts: uploads the nodes and the mixture table
 *                        (node_mix, or the bound one when NULL) and waits for
 *                        the bound mixtures' pending work.  Call it from one
 *                        thread after any change to the tree, the binding or
 *                        the bound mixtures (once per render pass); a later
 *                        change un-publishes the tree (context calls then fail
 *                        with SDMM_E_STATE).
 *   sdmm_guide_ctx_*     one render worker's context: its own HIP stream
 *                        (hip_stream NULL: a new non-blocking stream the
 *                        context owns) and its own guided-batch / product
 *                        scratch.  Contexts of one tree run at once from
 *                        different host threads with no lock; calls on ONE
 *                        context must be serialised by the caller.
 *   sdmm_ctx_guide_pdf_wavefront / sdmm_ctx_guide_product_wavefront
 *                        sdmm_guide_pdf_wavefront / sdmm_guide_product_wavefront
 *                        against the published tree on the context's stream
 *                        (outputs bitwise equal; asynchronous -- synchronise
 *                        the context's stream before reading them). */
typedef struct sdmm_guide_ctx sdmm_guide_ctx;
int sdmm_stree_publish(sdmm_stree* t, const sdmm_mix* const* node_mix);
int sdmm_guide_ctx_create(sdmm_stree* t, void* hip_stream, sdmm_guide_ctx** out);
void sdmm_guide_ctx_destroy(sdmm_guide_ctx* g);
void* sdmm_guide_ctx_stream(const sdmm_guide_ctx* g);
int sdmm_ctx_guide_pdf_wavefront(sdmm_guide_ctx* g, int64_t nq, const float* const c[3], const float* const u[3],
                                 const float* const dgiven[3], const uint8_t* pdf_mode, float* const d[3], float* pdf,
                                 int32_t* comp, int32_t* node_out);
int sdmm_ctx_guide_product_wavefront(sdmm_guide_ctx* g, int64_t nq, const float* const c[3], const float* const u[3],
                                     const float* choice, const float* const dgiven[3], const sdmm_bsdf_table* bsdf,
                                     const int32_t* material, const float* const frame[9], float* const d[3],
                                     float* pdf, int32_t* comp, float* heuristic, int32_t* node_out);
/* Several render workers' guided bounces served as ONE wavefront (round 6):
 * the requests' queries, in request order, go through a single
 * sdmm_ctx_guide_pdf_wavefront on the context -- each query's outputs are
 * bitwise those of a call on its own request (queries are independent) --
 * with the copies done here: per request one strided H2D of its nine query
 * planes and one of its mode bytes, one strided D2H of its four output planes
 * and one of its components.  Synchronous (the context's stream is
 * synchronised before returning).  Host buffers must be pinned
 * (hipHostMalloc / hipHostRegister): checked, SDMM_E_INVALID otherwise.  The
 * C++ mirror's sdmm_amd::GuideBatcher gathers concurrent workers' requests
 * into these calls.
 *   in   : planes c0 c1 c2 u0 u1 u2 dgiven0 dgiven1 dgiven2 (as
 *          sdmm_guide_pdf_wavefront), plane p at in + p * in_stride
 *   mode : n bytes (pdf_mode)
 *   out  : planes d0 d1 d2 pdf, plane p at out + p * out_stride
 *   comp : n int32 */
typedef struct sdmm_guide_host_req {
    int64_t n;
    const float* in;
    int64_t in_stride;
    const uint8_t* mode;
    float* out;
    int64_t out_stride;
    int32_t* comp;
} sdmm_guide_host_req;
int sdmm_ctx_guide_pdf_host_batch(sdmm_guide_ctx* g, int nreq, const sdmm_guide_host_req* reqs);
/* Page-locked host memory for such requests (hipHostMalloc / hipHostFree on
 * the library's side, so that host code needs no HIP headers). */
int sdmm_pinned_alloc(size_t bytes, void** out);
void sdmm_pinned_free(void* p);
/* Checkpoints (.asdmm, JSON; schema in DESIGN.md section 9).
 *   sdmm_save_json      the accelerator: sdmm::save_json(m_accelerator, path),
 *                       volpath_sdmm.cpp:117-126 (model_%05i.asdmm, once per
 *                       render iteration, :441).  Writes the tree's node table
 *                       and, for every node with a non-NULL node_mix entry
 *                       (node_mix may be NULL: tree only), that mixture's
 *                       canonical + derived arrays and its stepwise-EM state.
 *   sdmm_load_json      the inverse.  tree_out NULL: size query, only
 *                       *num_nodes_out is set.  Otherwise node_mix_out (cap >=
 *                       num_nodes) receives one new handle per saved mixture and
 *                       NULL elsewhere; restored mixtures are bitwise the saved
 *                       ones (guide outputs, later EM steps).  A malformed file
 *                       creates nothing and returns SDMM_E_INVALID.
 *   sdmm_mix_save_json / sdmm_mix_load_json   one mixture: jmm
 *                       MixtureModel::save/load (mixture_model.h:315-326).
 *   sdmm_get_em_params  the constructor arguments the handle was created with.
 *   sdmm_restore_params exact inverse of sdmm_get_params (every array required;
 *                       no MVTN::set re-derivation).
 *   sdmm_stree_set_nodes replace the node table (as sdmm_stree_get_nodes
 *                       returns it; children must follow their parent). */
int sdmm_save_json(const sdmm_stree* t, const sdmm_mix* const* node_mix, const char* path);
int sdmm_load_json(const char* path, int device, sdmm_stree** tree_out, sdmm_mix** node_mix_out, int cap,
                   int* num_nodes_out);
int sdmm_mix_save_json(const sdmm_mix* m, const char* path);
int sdmm_mix_load_json(const char* path, int device, sdmm_mix** out);
int sdmm_get_em_params(const sdmm_mix* m, sdmm_em_params* p);
/* A new handle holding a copy of m's mixture and stepwise EM state (device to
 * device, on m's stream; the new handle uses m's stream) -- a split leaf's
 * children start from their parent's distribution and optimizer (jmm
 * SNTree::createChildNode, sntree.h:172-205). */
int sdmm_clone(const sdmm_mix* m, sdmm_mix** out);
/* sdmm_clone of n handles of one K into one slab (on src[0]'s stream, or on
 * hip_stream: the new handles then use it). */
int sdmm_clone_many(const sdmm_mix* const* src, int n, sdmm_mix** out);
int sdmm_clone_many_on_stream(const sdmm_mix* const* src, int n, void* hip_stream, sdmm_mix** out);
/* dst[i] := src[i] (mixture + EM state), one kernel on dst[0]'s stream after
 * the sources' pending work -- sdmm::prepare(conditioner, sdmm) of the async
 * update (volpath_sdmm.cpp:227-242) when conditioners are separate handles. */
int sdmm_copy_many(const sdmm_mix* const* src, sdmm_mix* const* dst, int n);
int sdmm_restore_params(sdmm_mix* m, const sdmm_params_out* in);
int sdmm_stree_set_nodes(sdmm_stree* t, int n, const float* aabb, const int32_t* child, const int32_t* axis);

/* ---- Guided path tracing on the device (SDMMRenderer::Li) ----------------
 * An analytic scene of parallelograms (Mitsuba rectangles; a cube is six) and
 * an optional triangle mesh (sdmm_scene_desc's mesh fields; face normals) with
 * diffuse BSDFs, one-sided area emitters and an optional environment emitter
 * (a constant or a lat-long map: sdmm_scene_desc's env fields), rendered by a wavefront path
 * tracer whose every bounce goes through sdmm_guide_pdf_wavefront -- the
 * plugin's per-bounce sampleSurface / pdfSurface (sdmm_proc.cpp:275-590,
 * :592-871) on the device.  The Cornell Box of the test suite
 * (test-suite/scenes/cornell-box/cornell-box.xml:75-143) is this kind of
 * scene (sdmm-mitsuba_amd/scenes.py).
 *
 *   sdmm_scene_create   quads: 9 floats each (corner, edge1, edge2, world);
 *                       normal = normalize(edge1 x edge2), negated where
 *                       flip_normals[q] (nullable); bsdf[q] indexes
 *                       reflectance (3 per BSDF); emitter[q] (nullable, -1 =
 *                       none) indexes radiance (3 per emitter, Le on the
 *                       normal side); camera_to_world row major 4x4 (Mitsuba's
 *                       toWorld, camera looks along +z), fov along x.
 *   sdmm_scene_normalization  render() (volpath_sdmm.cpp:375-393): the scene
 *                       AABB without the camera gives scene_min and
 *                       spatial_norm = its largest extent (scene_norm.json),
 *                       the tree box = [0, extent / norm] -+ 1e-5 (getAABB).
 *   sdmm_li_render      spp samples for pixels [pixel_begin, pixel_end) (row
 *                       major), one path per sample; image (device, 3 planes
 *                       of width * height floats) receives each pixel's mean
 *                       radiance, image_sqr (nullable) the mean of the squared
 *                       samples (the reference's m_blockSqr, sdmm_wr.cpp:144).  guided = 0: BSDF sampling only (iteration
 *                       0, :311-323); otherwise every bounce queries the
 *                       leaves' mixtures (node_mix, or the table bound to t)
 *                       with the BSDF/guide choice of probability
 *                       bsdf_fraction (0.5, :383).  Conditions are
 *                       (p - scene_min) / spatial_norm (createCondition,
 *                       :263-273).  Runs on the tree's stream.  The saved
 *                       vertices (Li's Vertex records, :606-637, :815-846)
 *                       stay in the scene's buffers; *vertices_out (nullable)
 *                       points at them until the next sdmm_li_render.
 * Random numbers are counter based: sample (path, stream, dimension) of a
 * path are fixed, whatever runs beside it (render_device.h). */
typedef struct sdmm_scene sdmm_scene;
/* A glossy material's learned BSDF: the reference's BSDF::SDMM4
 * (include/mitsuba/render/bsdf.h:310-314), a mixture over (theta_i, alpha) x
 * direction loaded per material by sdmm::load_json (roughconductor.cpp:
 * 230-245).  M <= 8 components; host arrays
 *   weights[M]
 *   means[M][5]  (theta, alpha, x, y, z): the condition's mean and the unit
 *                direction in the canonical local frame (z = normal, wi at
 *                azimuth 0)
 *   covs[M][16]  row major over the tangent coordinates (theta, alpha, t1,
 *                t2), t at the component's direction in its
 *                Coordinates(mean) frame (sdmm_bsdf_table's convention).
 * getDMM (roughconductor.cpp:182-194) conditions it on (theta_i =
 * acos(min(1, cos theta_i)), alpha) with create_conditional_pruned(..., 2):
 * this library's reading of that sdmm-lib call (absent from the snapshot) is
 * in sdmm-mitsuba_amd/csrc/learned_bsdf.h and DESIGN.md section 10. */
typedef struct sdmm_learned_bsdf4 {
    int M;
    const float* weights;
    const float* means;
    const float* covs;
} sdmm_learned_bsdf4;
/* getDMM + rotate_to_wo on the host for the local incident direction
 * wi_local (wi_local[2] > 0; the plugin's learnedRow): *n_out (<= keep)
 * lobes weights[n], means[n][3] (local, unit), covs[n][4] (2x2 in each
 * mean's Coordinates frame); *n_out = 0: no valid conditional.  The device
 * render forms the same lobes bitwise. */
int sdmm_learned4_conditional(const sdmm_learned_bsdf4* m, float alpha, const float wi_local[3], int keep,
                              int* n_out, float* weights, float* means, float* covs);
/* The same for nq local incident directions on the device (wi_local: 3
 * device planes; outputs device: weights[nq][keep], means[nq][keep][3],
 * covs[nq][keep][4], n_out[nq] the lobes per query, unused lobes weight 0),
 * asynchronous on hip_stream -- a plugin's whole wavefront of getDMM calls
 * in one launch. */
int sdmm_learned4_conditional_device(const sdmm_learned_bsdf4* m, float alpha, int64_t nq,
                                     const float* const wi_local[3], int keep, float* weights, float* means,
                                     float* covs, int32_t* n_out, void* hip_stream);
/* sdmm::load_json / save_json of a learned BSDF (the material's .sdmm file,
 * roughconductor.cpp:230-245) in this library's JSON form (DESIGN.md section
 * 9): load with cap 0 is a size query (*M_out only); otherwise the arrays
 * hold cap components. */
int sdmm_learned4_save_json(const sdmm_learned_bsdf4* m, const char* path);
int sdmm_learned4_load_json(const char* path, int cap, int* M_out, float* weights, float* means, float* covs);
/* A learned BSDF over a condition of dimension C: C = 2 is the SDMM4 above,
 * C = 3 the reference's BSDF::SDMM5 (bsdf.h:316-324) -- Phong on (theta_i,
 * specWeight = max specular RGB, log max(1, exponent)) (phong.cpp:75-90),
 * rough dielectric and rough plastic on (theta_i, alpha, eta)
 * (roughdielectric.cpp:198-211, roughplastic.cpp:212-224).  M <= 8; host arrays
 *   weights[M]
 *   means[M][C+3]      the C condition means, then the unit direction
 *   covs[M][(C+2)^2]   row major over the tangent (c_0 .. c_{C-1}, t1, t2). */
typedef struct sdmm_learned_bsdf {
    int C;
    int M;
    const float* weights;
    const float* means;
    const float* covs;
} sdmm_learned_bsdf;
/* getDMM + rotate_to_wo for any of those materials on the host: the condition
 * is (theta_i = acos(min(1, wi_local[2])), cond_rest[0 .. C-2]).
 *   keep 1..8, force -1  sdmm::create_conditional_pruned(conditioner, condition,
 *                        dmm, keep) (roughconductor.cpp:192, roughdielectric.cpp:
 *                        209, roughplastic.cpp:222)
 *   keep 1..8, force f   the five-argument create_conditional_pruned(..., keep,
 *                        f) (phong.cpp:88, f = 1 the diffuse component):
 *                        component f, when its conditioned weight is > 0, is
 *                        always kept; f >= M: SDMM_E_INVALID
 *   keep 0               the unpruned sdmm::create_conditional (blendbsdf.cpp:
 *                        96): every valid component, in model order
 * Outputs as sdmm_learned4_conditional (room for 8 lobes when keep is 0); at
 * C = 2, force -1 they equal its outputs bitwise.  This library's reading of
 * those sdmm-lib calls (absent from the snapshot): csrc/learned_bsdf.h and
 * DESIGN.md section 10. */
int sdmm_learned_conditional(const sdmm_learned_bsdf* m, const float* cond_rest, const float wi_local[3], int keep,
                             int force, int* n_out, float* weights, float* means, float* covs);
/* The same for nq queries on the device, each with its own condition (a
 * wavefront's Phong hits carry different exponents): cond_rest holds C - 1
 * entries, entry i a device plane of nq values or NULL to broadcast the host
 * scalar cond_scalar[i].  Outputs device, R = keep (8 when keep is 0) lobes a
 * query: weights[nq][R], means[nq][R][3], covs[nq][R][4], n_out[nq]; unused
 * lobes weight 0.  Asynchronous on hip_stream; bitwise the host call's. */
int sdmm_learned_conditional_device(const sdmm_learned_bsdf* m, const float* const* cond_rest,
                                    const float* cond_scalar, int64_t nq, const float* const wi_local[3], int keep,
                                    int force, float* weights, float* means, float* covs, int32_t* n_out,
                                    void* hip_stream);
/* sdmm::save_json / load_json of such a model (phong.cpp:102-117): format
 * "sdmm-amd.sdmm5" with "C" (DESIGN.md section 9); the loader also reads an
 * "sdmm-amd.sdmm4" file as C = 2.  Load with cap 0 is a size query (*C_out,
 * *M_out only). */
int sdmm_learned_save_json(const sdmm_learned_bsdf* m, const char* path);
int sdmm_learned_load_json(const char* path, int cap, int* C_out, int* M_out, float* weights, float* means,
                           float* covs);
/* Phong::sample / eval / pdf (bsdfs/phong.cpp:171-289) on the host, as the
 * device Li runs them: params = the 8 bsdf_params floats of a kind-3 BSDF,
 * rho its diffuse reflectance, wi the local incident direction.  With u (2
 * uniforms): wo is sampled from them (out) and value = eval / pdf (sample's
 * return value; 0 with pdf 0 for a void sample); u NULL: wo is given and
 * value = eval (ESolidAngle).  pdf: the solid-angle pdf of wo. */
int sdmm_bsdf_phong_host(const float* params, const float rho[3], const float wi[3], const float* u, float wo[3],
                         float value[3], float* pdf);
/* RoughDielectric::sample / eval / pdf (bsdfs/roughdielectric.cpp: eval
 * :317-395, pdf :397-469, sample(bRec, pdf, sample) :560-662; isotropic
 * Beckmann, sampleVisible = false, ERadiance) on the host, as the device Li
 * runs them, with the semantics of sdmm_bsdf_phong_host: params = the 8
 * bsdf_params floats of a kind-4 BSDF, spec_trans its specularTransmittance,
 * wi the local incident direction (wi.z < 0: a hit from inside; wi.z == 0
 * gives 0).  With u (3 uniforms: the microfacet normal's two, then the lobe
 * choice that the reference draws with bRec.sampler->next1D(), reflection
 * when u[2] <= F): wo is sampled (out), value = sample's return value (0 with
 * pdf 0 for a void sample: microfacet pdf 0, a failed side check, cosThetaT ==
 * 0) and *eta_out = bRec.eta, the relative index the sample crossed (1 on
 * reflection, eta entering, 1 / eta leaving; 1 for a void sample).  u NULL:
 * wo is given (either side), value = eval (ESolidAngle), and *eta_out what
 * sample would have set for that wo: 1 if wi.z * wo.z > 0, else eta for wi.z
 * > 0 and 1 / eta for wi.z < 0 -- the library's reading for a guide-chosen
 * direction, where the reference multiplies the path's eta by a bRec.eta that
 * BSDFSamplingRecord's constructor never initialises (records.inl:24-27).
 * pdf: the solid-angle pdf of wo.  Inputs and outputs are floats; between
 * them the arithmetic is double (the float32 formulas miss their float64
 * values by 1e-4 .. 2e-3 where they cancel: DESIGN.md section 10). */
int sdmm_bsdf_roughdielectric_host(const float* params, const float spec_trans[3], const float wi[3], const float* u,
                                   float wo[3], float value[3], float* pdf, float* eta_out);
/* The same over nq queries on device planes (SoA), asynchronous on
 * hip_stream, each query bitwise the host call's: wi[3] the incident planes;
 * u[3] the uniforms' planes (sample mode: wo[3] is written) or NULL (eval
 * mode: wo[3] is read); value[3], pdf and eta_out planes of nq floats. */
int sdmm_bsdf_roughdielectric_device(const float* params, const float spec_trans[3], int64_t nq,
                                     const float* const wi[3], const float* const* u, float* const wo[3],
                                     float* const value[3], float* pdf, float* eta_out, void* hip_stream);
/* The two delta-only BSDFs on the host, as the device Li runs them, with the
 * semantics of sdmm_bsdf_roughdielectric_host; the call dispatches on
 * params[0].  Kind 5, SmoothDielectric (bsdfs/dielectric.cpp: sample
 * :277-333, eval :228-253, pdf :255-275; ERadiance, both components):
 * spec_trans its specularTransmittance, wi.z < 0 a hit from inside, wi.z == 0
 * gives 0.  Kind 6, SmoothConductor (bsdfs/conductor.cpp:223-285): one-sided
 * (wi.z <= 0 gives 0), spec_trans not read (may be NULL).
 * With u (2 uniforms, the reference's sample; only u[0] is read): kind 5
 * reflects when u[0] <= F (so always at a total internal reflection, F = 1) --
 * wo = reflect(wi), value = specularReflectance, pdf = F, *eta_out = 1 -- and
 * transmits otherwise: wo = refract(wi, cosThetaT), value =
 * specularTransmittance * factor^2 with factor = 1 / eta entering and eta
 * leaving, pdf = 1 - F, *eta_out = eta entering, 1 / eta leaving.  Kind 6: wo
 * = reflect(wi), value = specularReflectance * fresnelConductorExact(cos
 * theta_i, eta, k), pdf 1, *eta_out 1.  A zero value comes with its lobe's wo
 * and pdf, except for wi.z == 0 and the conductor's back side (wo = +z, pdf
 * 0).  u NULL: wo is given and value / pdf are the reference's eval / pdf
 * under EDiscrete -- the lobe's value times its probability (reflectance * F,
 * transmittance * factor^2 * (1 - F), the conductor's value) and that
 * probability where |dot(lobe direction, wo) - 1| <= DeltaEpsilon = 1e-3, 0
 * elsewhere; *eta_out what sample sets for the lobe on wo's side.  Floats in
 * and out, double in between, as the rough dielectric's pair. */
int sdmm_bsdf_smooth_host(const float* params, const float spec_trans[3], const float wi[3], const float* u,
                          float wo[3], float value[3], float* pdf, float* eta_out);
/* The same over nq queries on device planes (SoA), asynchronous on
 * hip_stream, each query bitwise the host call's: u[2] the uniforms' planes
 * (sample mode; u[1] must be set and is not read) or NULL (eval mode). */
int sdmm_bsdf_smooth_device(const float* params, const float spec_trans[3], int64_t nq, const float* const wi[3],
                            const float* const* u, float* const wo[3], float* const value[3], float* pdf,
                            float* eta_out, void* hip_stream);
/* An RGB bitmap texture (<texture type="bitmap">, textures/bitmap.cpp) for
 * sdmm_scene_desc.textures.  pixels: host array [height][width][3] of linear
 * RGB floats, texel (x, y) at 3 * (y * width + x), row 0 is v = 0 -- no flip,
 * no gamma, no fromLinearRGB: the caller decodes.  filter: 0 bilinear
 * (MIPMap::evalBilinear on level 0; also what the reference's EWA and
 * trilinear textures take without ray differentials), 1 nearest (evalBox).
 * wrap_u, wrap_v: 0 repeat, 1 clamp, 2 mirror, 3 zero, 4 one (wrapModeU /
 * wrapModeV; evalTexel, render/mipmap.h:503-563).  uv_scale, uv_offset: the
 * lookup is at its.uv * uv_scale + uv_offset (librender/texture.cpp:112-121);
 * a uv_scale of 0 is rejected, so that a texture zeroed except for its size
 * and pixels is not valid by accident (Mitsuba's default is 1). */
typedef struct {
    int width, height;
    const float* pixels;
    int filter;
    int wrap_u, wrap_v;
    float uv_scale[2];
    float uv_offset[2];
} sdmm_texture;
typedef struct {
    int n_quads;
    const float* quads;
    const int32_t* flip_normals;
    const int32_t* bsdf;
    int n_bsdfs;
    const float* reflectance;
    const int32_t* emitter;
    int n_emitters;
    const float* radiance;
    float camera_to_world[16];
    float fov_x_deg;
    float near_clip;
    int width, height;
    /* nullable (every BSDF diffuse): 8 floats per BSDF -- [0] kind (0
     * diffuse, 1 smooth plastic: bsdfs/plastic.cpp, its diffuseReflectance in
     * `reflectance`), [1..3] specularReflectance, [4] eta = intIOR / extIOR,
     * [5] 1 / eta^2, [6] fdrInt (the internal diffuse Fresnel reflectance,
     * fresnelDiffuseReflectance(1 / eta)), [7] the specular sampling weight
     * sAvg / (dAvg + sAvg) (plastic.cpp:188-196).  A plastic bounce queries
     * the guide like any BSDF with a smooth lobe; a delta lobe chosen by the
     * BSDF sample returns weight / h with pdf * h and saves no vertex
     * (sdmm_proc.cpp:297, :383-409, :764).  Kind 2, rough conductor
     * (bsdfs/roughconductor.cpp; `reflectance` unused): [1..3]
     * specularReflectance, [4] eta, [5] k (a gray conductor), [6] the
     * Beckmann alpha (isotropic, sampleVisible = false), [7] unused.  Kind 3,
     * modified Phong (bsdfs/phong.cpp; its diffuseReflectance in
     * `reflectance`, both reflectances after configure()'s energy scaling):
     * [1..3] specularReflectance, [4] exponent, [5] the specular sampling
     * weight sAvg / (dAvg + sAvg) (phong.cpp:146-148), [6], [7] unused.
     * Kind 4, rough dielectric (bsdfs/roughdielectric.cpp; its
     * specularTransmittance in `reflectance`): [1..3] specularReflectance,
     * [4] eta = intIOR / extIOR (> 0 and != 1), [5] 1 / eta, [6] the Beckmann
     * alpha (isotropic, sampleVisible = false), [7] unused.  Its quads are
     * two-sided: a path meeting one from behind is inside the medium, the
     * BSDF runs in Frame(n) of the stored normal, the saved vertex carries -n
     * (sdmm_proc.cpp:765-767), and the path's relative index (Russian
     * roulette, :864) is multiplied by the index each bounce crossed -- for a
     * guide-chosen direction by what sample would have set for it (see
     * sdmm_bsdf_roughdielectric_host).
     * Kind 5, smooth dielectric (bsdfs/dielectric.cpp; its
     * specularTransmittance in `reflectance`): [1..3] specularReflectance,
     * [4] eta = intIOR / extIOR (> 0 and != 1), [5] 1 / eta, [6], [7] unused;
     * two-sided like kind 4.  Kind 6, smooth conductor (bsdfs/conductor.cpp;
     * `reflectance` unused): [1..3] specularReflectance, [4] eta, [5] k (a
     * gray conductor, as kind 2), [6], [7] unused; one-sided.  Both are delta
     * only (sdmm_bsdf_smooth_host): a bounce on one takes the BSDF's sample
     * with pdf = bsdfPdf, queries no guide (it is not counted in
     * guided_queries and takes no row of the product's table), saves no
     * vertex and still advances the depth (sdmm_proc.cpp:297-302, :764);
     * radiance found after it reaches the vertices saved before it.  The lobe
     * choice is dimension 0 of the bounce's stream; the path's relative index
     * takes the crossed eta as for kind 4.  A learned_models /
     * learned_models_nd entry on such a BSDF is not read, nor validated.  Not supported on
     * these kinds: textures, a spectral (per-channel) eta or k, the thin
     * dielectric, and the reference's ENull passage through index-matched
     * interfaces (eta == 1 is rejected). */
    const float* bsdf_params;
    /* nullable: n_bsdfs entries (appended in round 6) -- a rough conductor's
     * learned BSDF, the material's SDMM4 (roughconductor.cpp:182-194,
     * :230-245); M = 0 (or the array NULL): none, so getDMM fails and the
     * product falls back to the plain conditional (sdmm_proc.cpp:327-392).
     * Only rough conductors read theirs. */
    const struct sdmm_learned_bsdf4* learned_models;
    /* nullable: n_bsdfs entries (appended after learned_models; the
     * zero-initialise rule below covers older callers) -- the learned BSDFs
     * over a C-dimensional condition.  Phong BSDFs (kind 3) read theirs: the
     * material's SDMM5 (phong.cpp:75-90, :102-117), C = 3 and M >= 2 (the
     * forced diffuse component is index 1); so do rough dielectrics (kind 4):
     * the SDMM5 over (theta_i, alpha, eta) (roughdielectric.cpp:198-211), C =
     * 3 and M >= 1, conditioned on hits from outside only.  M = 0 (or the
     * array NULL): none. */
    const struct sdmm_learned_bsdf* learned_models_nd;
    /* A triangle mesh beside the quads (appended after learned_models_nd; the
     * zero-initialise rule below covers older callers: n_triangles = 0 and
     * every rule above holds, the other mesh fields are then not read).
     *   mesh_vertices     3 floats per vertex in world space (the caller
     *                     applies toWorld), n_mesh_vertices of them
     *   triangles         3 vertex indices per triangle, n_triangles of them
     *   tri_bsdf          required with triangles: indexes the same BSDF
     *                     tables as bsdf[q]; any kind, the two-sided 4 included
     *   tri_emitter       nullable, -1 = none: indexes radiance, one-sided as
     *                     for quads (radiance and n_emitters are required
     *                     when it is set, also without a quad `emitter`)
     *   tri_flip_normals  nullable
     * The normal is the face normal normalize((p1 - p0) x (p2 - p0)), negated
     * where flipped (vertex normals: mesh_normals below; UVs and textures:
     * mesh_uvs below).  Instancing is not supported.  n_quads may be 0 with triangles.
     * Primitive ids: quads 0 .. n_quads-1, triangle i is n_quads + i; the
     * learned-BSDF row of a hit is still its bsdf index, and the scene AABB
     * of sdmm_scene_normalization includes every mesh vertex.
     * SDMM_E_INVALID (with a message): a vertex index out of range, a
     * non-finite vertex, a zero-area triangle (cross product of length 0 in
     * float), a material or emitter index out of range, more than 2^26
     * triangles, a BVH deeper than the traversal stack (24 inner levels: what
     * a median-split tree of 2^26 triangles needs, so a valid mesh always
     * fits). */
    int n_mesh_vertices;
    const float* mesh_vertices;
    int n_triangles;
    const int32_t* triangles;
    const int32_t* tri_bsdf;
    const int32_t* tri_emitter;
    const int32_t* tri_flip_normals;
    /* An environment emitter (appended after tri_flip_normals; the
     * zero-initialise rule below covers older callers: env_kind = 0, no
     * environment, the other env fields are then not read and everything
     * behaves as before).  A ray that leaves the scene -- the camera ray or
     * any bounce ray, delta lobes and rays leaving a dielectric included --
     * returns throughput * evalEnvironment(ray) (sdmm_proc.cpp:659-671,
     * :1047-1051) and ends the path.
     *   env_kind            0 none; 1 constant (emitters/constant.cpp:
     *                       env_radiance, whatever the direction); 2 a
     *                       lat-long map (emitters/envmap.cpp:380-393, :409)
     *   env_radiance        kind 1: returned as is (no scale, no transform)
     *   env_width, env_height, env_pixels
     *                       kind 2: host array [height][width][3], linear RGB;
     *                       row 0 is the +y pole of the emitter's local frame
     *                       (v = 0 where acos(v.y) = 0), u = atan2(v.x, -v.z)
     *                       / 2 pi wraps horizontally, v clamps
     *   env_scale           kind 2: m_scale, multiplies the lookup
     *   env_world_to_local  kind 2: the linear part of toWorld.inverse(), row
     *                       major, applied to the ray direction as given (no
     *                       renormalisation)
     * Every ray takes the bilinear lookup of the finest level (MIPMap::
     * evalBilinear, render/mipmap.h:575-596): there are no ray differentials
     * here, so not the EWA-filtered lookup Mitsuba gives its camera rays
     * (envmap.cpp:394-407).  A direction whose texture coordinates are not
     * finite returns 0.  The scene AABB and sdmm_scene_normalization do not
     * change (an environment has no extent), nor does the rule for what
     * geometry a scene must hold.
     * SDMM_E_INVALID (with a message): a kind outside 0..2; kind 2 with a NULL
     * map, a width or height < 1 or more than 2^26 texels; a non-finite or
     * negative radiance, texel or scale; a non-finite matrix entry. */
    int env_kind;
    float env_radiance[3];
    int env_width, env_height;
    const float* env_pixels;
    float env_scale;
    float env_world_to_local[9];
    /* nullable: n_bsdfs entries, 0 or 1 (appended after env_world_to_local;
     * the zero-initialise rule below covers older callers: NULL or all zeros
     * and every rule above holds).  1 on BSDF b: b is the single-child
     * <bsdf type="twosided"> (bsdfs/twosided.cpp, m_nestedBRDF[1] =
     * m_nestedBRDF[0], :90-91) around the BSDF its row describes.  A hit with
     * wi . n < 0 on such a BSDF (n the stored face normal, Frame(n) = (s, t,
     * n)) is live: the bounce runs in the frame (s, t, -n) -- local wi =
     * (wi.s, wi.t, -(wi.n)), the nested BSDF's sample, eval and pdf on it
     * unchanged, a local w to world as s w0 + t w1 - n w2 (wi.z *= -1 ...
     * wo.z *= -1, :111-137, :191-213; not Frame(-n), whose tangents differ),
     * a guide-chosen direction evaluated the same way; getEta() = 1 (:244),
     * so the path's relative index is untouched; the saved vertex carries -n
     * (sdmm_proc.cpp:765-767).  With sample_product the learned model is
     * conditioned on the flipped local wi and the query's frame is F = [s t
     * -n], which is getDMM's negated column 2 of `to` and mean.z (:151-159)
     * under the integrator's [s t n] (sdmm_proc.cpp:344-354); a diffuse row
     * sees the flipped normal as F's third column (:306-308, :335-339); kind 1
     * has no getDMM and keeps the plain conditional.  wi . n == 0 and zero
     * reflectances end the path as before; kind 6 stays delta only (no query,
     * no vertex, the depth advances), now from both sides; a front hit is
     * bitwise what it is without the flag; an area emitter stays one-sided
     * whatever its primitive's BSDF (emitters/area.cpp).
     * SDMM_E_INVALID (with a message): an entry other than 0 or 1; a 1 on a
     * kind-4 or kind-5 BSDF ("Only materials without a transmission component
     * can be nested", :106-108).
     * Not supported: the two-child form (m_nestedBRDF[1] != [0]; there getDMM
     * always asks child 0, :146), two-sided emitters (with
     * mesh_normals the stored normal n above is the hit's shading normal ns); the Mitsuba plugin does not run the device Li, so
     * it takes no such flag. */
    const int32_t* bsdf_twosided;
    /* nullable: vertex normals of the mesh, 3 floats per mesh vertex in world
     * space (appended after bsdf_twosided; the zero-initialise rule below
     * covers older callers: NULL and every rule above holds, bit for bit).
     * The values are used as given: vertex normals are not normalised, the
     * interpolated sum is (render/skdtree.h:388).  At a hit on triangle (i0,
     * i1, i2) with the triangle test's own u, v:
     *   b  = (1 - u - v, u, v)
     *   ns = normalize(n[i0] b.x + n[i1] b.y + n[i2] b.z), negated where
     *        tri_flip_normals is set (Mitsuba's per-mesh flipNormals negates
     *        the vertex normals, trimesh.cpp:624-628; the winding is left
     *        alone when normals are present)
     *   ng = the winding's face normal normalize((p1 - p0) x (p2 - p0)),
     *        without the flip, negated when dot(ng, ns) < 0 (skdtree.h:390-396)
     * Everything the Li did on the face normal it does on ns: the side tests
     * (cos_i, the two-sided back hit, inside a dielectric), Frame(ns) for
     * every toLocal / toWorld, the cosine pdfs, the product's F = [s t +-ns]
     * and the learned conditionals' local wi, the guide's condition normal
     * and the saved vertex's normal (fields 13-15; -ns behind a two-sided BSDF
     * or inside a dielectric), and an emitting triangle is seen where
     * dot(ns, d) < 0 (emitters/area.cpp:105).  ng appears only in the
     * strictNormals tests (sdmm_li_params.non_strict_normals).  Quads, and a
     * mesh without mesh_normals, keep ns = ng = the face normal.
     * Documented choices: the shading frame stays Frame(ns) (coordinateSystem)
     * and is not Mitsuba's computeShadingFrame(ns, dpdu) -- all seven BSDF
     * kinds are isotropic, so the tangents only move bits; the sum is divided
     * by its length where Mitsuba multiplies by the reciprocal, so exact
     * axis-aligned vertex normals reproduce the face normal bit for bit; and
     * where the interpolated sum has length 0 or is not finite, ns = ng = the
     * face normal (flip applied) as without normals -- Mitsuba would carry a
     * NaN there.
     * SDMM_E_INVALID (with a message): mesh_normals set without triangles; a
     * non-finite normal; a normal of length 0 (all three components 0). */
    const float* mesh_normals;
    /* Bitmap textures on reflectances (every field below is appended after
     * mesh_normals; the zero-initialise rule below covers older callers: all
     * NULL / 0 and every rule above holds, bit for bit, with the kernels a
     * scene launched before).
     *   mesh_uvs      nullable: texture coordinates of the mesh, 2 floats per
     *                 mesh vertex.  At a hit on triangle (i0, i1, i2) with the
     *                 triangle test's own u, v: its.uv = t[i0] b.x + t[i1] b.y
     *                 + t[i2] b.z, b = (1 - u - v, u, v); without mesh_uvs
     *                 its.uv = (u, v) (render/skdtree.h:399-405).  On a quad
     *                 its.uv = (a, b), the two parametric coordinates of the
     *                 hit along e1 and e2, p0 at (0, 0) (shapes/rectangle.cpp:
     *                 163 with p0 as the local (-1, -1) corner).
     *   n_textures, textures
     *                 the scene's bitmaps (sdmm_texture above)
     *   bsdf_texture  nullable: n_bsdfs entries, the texture that replaces
     *                 BSDF b's reflectance row at every hit, -1 = none.  The
     *                 row is diffuse.cpp's reflectance (kind 0) and the
     *                 diffuseReflectance of plastic.cpp (kind 1) and phong.cpp
     *                 (kind 3); the value is Texture2D::eval(its, false)
     *                 (librender/texture.cpp:112-121: uv * uv_scale +
     *                 uv_offset) over BitmapTexture::eval(uv) (textures/
     *                 bitmap.cpp:431-454): MIPMap::evalBilinear, or evalBox
     *                 with the nearest filter, on the full-resolution level
     *                 (render/mipmap.h:503-596).  A hit whose texel is black
     *                 (with a zero specular reflectance) ends the path, as a
     *                 zero reflectance row does.
     * The constant bsdf_params stay the caller's: Phong's and plastic's
     * specular sampling weights come from the texture's average
     * (phong.cpp:146-148), as does configure()'s energy scaling.  Phong's
     * learned condition reads the specular reflectance and the exponent
     * (phong.cpp:82-84), neither textured here: product sampling is unchanged.
     * Departures: every hit takes eval(uv) -- there are no ray differentials
     * here, so not the EWA lookup Mitsuba gives its camera rays (bitmap.cpp:
     * 486); a non-finite uv gives 0 (evalBilinear's guard) in nearest mode
     * too; a texel coordinate that does not fit int32 gives 0 (floorToInt is
     * undefined there).
     * Not supported: a textured specular reflectance, exponent, alpha or
     * radiance; EWA / trilinear filtering; computeShadingFrame's UV tangents
     * (the shading frame stays Frame(ns)); procedural textures; image-file
     * reading.
     * SDMM_E_INVALID (with a message; these checks come after every other):
     * mesh_uvs without triangles or with a non-finite value; n_textures < 0
     * or textures NULL with n_textures > 0; bsdf_texture without textures; a
     * texture with width or height < 1, NULL pixels, an unknown filter or
     * wrap, a zero or non-finite uv_scale, a non-finite uv_offset, a
     * non-finite or negative texel; more than 2^26 texels in all; a
     * bsdf_texture entry outside -1 .. n_textures - 1, or set on a BSDF of
     * kind 2 (its row is unused) or 4, 5, 6 (which carry no textures).
     * (The reference reads any bitmap, negative and non-finite values
     * included; rejecting those here is this library's choice, the one it
     * makes for the environment map's texels and the reflectance rows.) */
    const float* mesh_uvs;
    int n_textures;
    const sdmm_texture* textures;
    const int32_t* bsdf_texture;
} sdmm_scene_desc;
/* The descriptor has grown across ABI revisions (bsdf_params was appended):
 * zero-initialise it (`sdmm_scene_desc d = {0};` / `memset`) before filling
 * the fields you use, so an older caller's unset trailing pointer is NULL --
 * sdmm_scene_create reads every field. */
typedef struct {
    int spp;
    int max_depth;            /* maxDepth (:649, :684), -1 = unbounded (capped by the vertex slots) */
    int rr_depth;             /* rrDepth (:858) */
    int guided;
    float bsdf_fraction;      /* heuristicConditionalWeight (0.5) */
    int saved_vertices;       /* vertex slots per path (>= max_depth - 1; the reference's array holds 10) */
    uint64_t seed;
    int64_t pixel_begin, pixel_end;
    /* sampleProduct (volpath_sdmm.cpp:60, sdmm_proc.cpp:327-392): guided
     * bounces sample the product of the leaf's conditional with the hit
     * material's learned BSDF (learned_bsdf row = the quad's bsdf index; for
     * a diffuse BSDF set diffuse[b], the plugin's slice-0 rule) through
     * sdmm_guide_product_wavefront, with h = 0.3 (0.5 when the product is
     * unusable) and the BSDF/guide choice taken against that h.  A rough
     * conductor's row is not read: each bounce conditions the conductor's
     * learned model (sdmm_scene_desc.learned_models: getDMM on theta_i and
     * alpha, pruned to 2 lobes -- none or no valid conditional: the plain
     * conditional) then rotate_to_wo(wi) and the shading frame to world,
     * sdmm_proc.cpp:340-355; the component index is then k * max(M, 2) + j
     * with a conductor or a Phong BSDF in the scene.  A Phong BSDF likewise
     * conditions its SDMM5 (sdmm_scene_desc.learned_models_nd: getDMM on
     * theta_i, the largest specular channel and log max(1, exponent), pruned
     * to 2 with the diffuse component 1 forced, phong.cpp:75-90), and a rough
     * dielectric its SDMM5 on (theta_i, alpha, eta), pruned to 2, for hits
     * from outside (roughdielectric.cpp:198-211; from inside, without a model
     * or a valid conditional: the plain conditional, h 0.5).  0: the plain
     * conditional with bsdf_fraction.  (bsdfOnly never trains, :416, so it
     * is the guided = 0 render; its learned-BSDF branch, :331/:384/:410, is
     * unreachable in the reference.) */
    int sample_product;
    sdmm_bsdf_table learned_bsdf;   /* device arrays */
    /* strictNormals (volpath_sdmm.cpp:54; appended: a zero-initialised struct
     * is the reference's default, strictNormals = true, and today's
     * behaviour).  0: a bounce ends where the incident direction lies on
     * different sides of the two normals, (wi . ng)(wi . ns) < 0, tested after
     * the depth test and before any BSDF sample (sdmm_proc.cpp:688-691), and
     * where the sampled direction does, (wo . ng) cosTheta(bRec.wo) <= 0
     * (:777-780; bRec.wo is in its.shFrame also behind a two-sided BSDF,
     * twosided.cpp:137, so the product is (wo . ng)(wo . ns)).  Not 0:
     * neither test runs; a zero or non-finite weight still ends the path.
     * Without sdmm_scene_desc.mesh_normals ns = ng, the first test never
     * fires, the second is cos^2 > 0 as it always was, and the field is not
     * read. */
    int non_strict_normals;
} sdmm_li_params;
/* Vertex records of the last render (device): field f of vertex v of path p
 * at rec[(f * max_vertices + v) * n_paths + p]; f: 0-2 weight (RGB), 3-5
 * throughput, 6 clamped sampling pdf, 7-12 point (condition, world
 * direction), 13-15 normal; nv[p] vertices per path; path p's global index
 * (the RNG's path counter) is path0 + p. */
typedef struct {
    int64_t n_paths;
    int max_vertices;
    int64_t path0;
    const float* rec;
    const int32_t* nv;
} sdmm_path_vertices;
typedef struct {
    int64_t paths;           /* paths started (pixels x spp) */
    int64_t segments;        /* bounce rays traced after the camera rays (a delta lobe's saves no vertex) */
    int64_t guided_queries;  /* live bounces that queried the guide (compacted wavefront sizes summed) */
    int64_t fallback_queries;   /* of those, served by the full-K path (the candidate list overflowed) */
} sdmm_li_stats;
int sdmm_scene_create(const sdmm_scene_desc* desc, int device, sdmm_scene** out);
void sdmm_scene_destroy(sdmm_scene* s);
int sdmm_scene_normalization(const sdmm_scene* s, float scene_min[3], float* spatial_norm, float tree_min[3],
                             float tree_max[3]);
int sdmm_li_render(sdmm_scene* s, sdmm_stree* t, const sdmm_mix* const* node_mix, const sdmm_li_params* p,
                   float* image, float* image_sqr, sdmm_path_vertices* vertices_out, sdmm_li_stats* stats);
/* The closest hit of nq rays against the scene's quads and triangles, as the
 * Li kernels find it: o, d three device planes each (origin, direction; the
 * direction need not be unit), prim[nq] the hit's primitive id or -1, t[nq]
 * its distance (maxt without a hit).  Asynchronous on hip_stream.
 * The closest-hit rule: t in (mint, maxt), the smallest t wins, on exactly
 * equal t the lowest primitive id.  mode 0 walks the triangles' BVH (built
 * on the host at sdmm_scene_create: binned SAH, leaves of at most 4, 64-byte
 * nodes holding both children's boxes; the walk visits every subtree whose
 * entry distance is not greater than the current best, so ties are seen),
 * mode 1 loops over all triangles with the same triangle test
 * (Triangle::rayIntersect, core/triangle.h:109-145); the quads go through
 * their loop in both.  Both modes, here and on the host, are meant to return
 * bitwise the same (prim, t): the walk's cull carries a margin (1e-4
 * relative) against the triangle test's rounding, so this is tested inside
 * an envelope ("Mesh: tested envelope": origins up to about 1e6
 * triangle sizes away), not proven for every input. */
int sdmm_scene_intersect(const sdmm_scene* s, int64_t nq, const float* const o[3], const float* const d[3], float mint,
                         float maxt, int mode, int32_t* prim, float* t, void* hip_stream);
/* The same entirely on the host (no HIP call: runs without a GPU) from a
 * description -- o, d host arrays [nq][3]; camera and film fields are not
 * read.  Validates as sdmm_scene_create does, builds the same BVH and walks
 * it with the same traversal source. */
int sdmm_scene_intersect_host(const sdmm_scene_desc* desc, int64_t nq, const float* o, const float* d, float mint,
                              float maxt, int mode, int32_t* prim, float* t);
/* The same over a BVH whose inner levels are capped at max_levels (0: the
 * traversal stack's 24, sdmm_scene_intersect_host's tree; a smaller cap as in
 * sdmm_mesh_bvh_dump).  The hits do not depend on the cap. */
int sdmm_scene_intersect_host_levels(const sdmm_scene_desc* desc, int max_levels, int64_t nq, const float* o,
                                     const float* d, float mint, float maxt, int mode, int32_t* prim, float* t);
/* sdmm_scene_intersect extended by the hit's two normals as the Li kernels
 * compute them (sdmm_scene_desc.mesh_normals): ns, ng three device planes
 * each, the shading and the geometric normal, zeros on a miss; on a quad, or
 * on a triangle of a mesh without vertex normals, both are the face normal
 * (flip applied).  Asynchronous on hip_stream. */
int sdmm_scene_shading(const sdmm_scene* s, int64_t nq, const float* const o[3], const float* const d[3], float mint,
                       float maxt, int mode, int32_t* prim, float* t, float* const ns[3], float* const ng[3],
                       void* hip_stream);
/* The same entirely on the host (no HIP call: runs without a GPU) from a
 * description -- o, d host arrays [nq][3], ns, ng host arrays [nq][3].
 * Validates as sdmm_scene_create does; one source (csrc/shading_normal.h)
 * serves this entry, the device entry and the Li kernels, bitwise alike. */
int sdmm_scene_shading_host(const sdmm_scene_desc* desc, int64_t nq, const float* o, const float* d, float mint,
                            float maxt, int mode, int32_t* prim, float* t, float* ns, float* ng);
/* sdmm_scene_intersect extended by the hit's texture coordinates and the
 * effective reflectance of its BSDF, as the Li kernels compute them
 * (sdmm_scene_desc.mesh_uvs, textures, bsdf_texture): uv two device planes
 * (its.uv, before uv_scale and uv_offset), rgb three -- the texture's value at
 * the hit, or the BSDF's reflectance row where it carries no texture (the uv
 * is reported all the same); zeros on a miss.  Asynchronous on hip_stream.
 * (A scene with triangles created with neither mesh_uvs nor textures holds no
 * per-triangle table: a hit on its mesh then finds its triangle by a linear
 * search -- the same answer, slowly.) */
int sdmm_scene_texture(const sdmm_scene* s, int64_t nq, const float* const o[3], const float* const d[3], float mint,
                       float maxt, int mode, int32_t* prim, float* t, float* const uv[2], float* const rgb[3],
                       void* hip_stream);
/* The same entirely on the host (no HIP call: runs without a GPU) from a
 * description -- o, d host arrays [nq][3], uv [nq][2], rgb [nq][3].  Validates
 * the geometry and the texture fields as sdmm_scene_create does (bsdf_params
 * is read for the kinds only); one source (csrc/texture.h) serves this entry,
 * the device entry and the Li kernels, bitwise alike. */
int sdmm_scene_texture_host(const sdmm_scene_desc* desc, int64_t nq, const float* o, const float* d, float mint,
                            float maxt, int mode, int32_t* prim, float* t, float* uv, float* rgb);
/* evalEnvironment of the scene's environment emitter (sdmm_scene_desc's env
 * fields) for nq directions: d, rgb three device planes each (the direction
 * is used as given; rgb: the radiance, 0 for a scene without an environment).
 * Asynchronous on hip_stream.  The Li kernels run the same lookup where a ray
 * leaves the scene. */
int sdmm_env_eval(const sdmm_scene* s, int64_t nq, const float* const d[3], float* const rgb[3], void* hip_stream);
/* The same entirely on the host (no HIP call: runs without a GPU) from a
 * description -- d, rgb host arrays [nq][3]; only the env fields are read,
 * and validated as sdmm_scene_create validates them.  Bitwise the device's. */
int sdmm_env_eval_host(const sdmm_scene_desc* desc, int64_t nq, const float* d, float* rgb);
/* Debug view of the BVH built for desc's mesh (host only).  max_levels: the
 * cap on inner levels (0: the traversal stack's 24; a smaller cap forces
 * median splits, and SDMM_E_INVALID when even those do not fit).  *n_nodes,
 * *levels (nullable) always; with cap_nodes >= *n_nodes also boxes[n][2][2][3]
 * (child, lo / hi, axis), children[n][2] (>= 0 an inner node, < 0 a leaf: ~c
 * = first * 8 + count into the leaf order) and order[n_triangles] (leaf order
 * -> triangle index).  cap_nodes 0: a size query. */
int sdmm_mesh_bvh_dump(const sdmm_scene_desc* desc, int max_levels, int* n_nodes, int* levels, int cap_nodes,
                       float* boxes, int32_t* children, int32_t* order);

/* Training-data producer: the tail of Li (sdmm_proc.cpp:876-965) for a batch
 * of paths' saved vertices.  Per path, vertices nv-1 down to
 * max(nv - saved_per_path, 0): the vertex's leaf (STree.find with its box,
 * :921-930) gets (point, normal, average weight) plus a stats entry when the
 * average is finite (push_back_data, :880-914); then 1 (last vertex) + 1
 * (average > 1000) jittered copies go to the leaf at point + (u - 1/2) x leaf
 * diagonal, a draw outside the tree or in the same leaf retried while fewer
 * than 8 draws failed (:932-964); u from stream 1024 + vertex of the path's
 * counter RNG under `seed`.  Output (device planes, capacity records): the
 * records in leaf order, a leaf's records in (path, push) order; node = leaf
 * id, source = p * max_vertices + v, stats = 1 for the vertex's own leaf.
 * *n_out = number of records (also when it exceeds capacity: then nothing is
 * written and SDMM_E_INVALID is returned; out NULL: count only); seg (host, nullable,
 * num_nodes + 1): leaf v's records are [seg[v], seg[v+1]).  lost (nullable):
 * visited vertices outside the tree or at a NaN position (the reference
 * throws), whatever their weight.  seg and lost are reported by a WRITING call
 * only: a count-only call (out NULL) leaves seg untouched and sets *lost to 0
 * although vertices may have been lost, and so does a call that returns
 * SDMM_E_INVALID for its capacity.  n_paths = 0: *n_out = 0, seg all zero,
 * *lost = 0.  The planes normal, stats, node and source of `out` are
 * nullable; x and w are required once there is a record to write.
 * Synchronous. */
typedef struct {
    float* x[6];
    float* normal[3];        /* nullable (all three) */
    float* w;
    uint8_t* stats;          /* nullable */
    int32_t* node;           /* nullable */
    int64_t* source;         /* nullable */
    int64_t capacity;
} sdmm_training_out;
int sdmm_push_training(sdmm_stree* t, const sdmm_path_vertices* v, int saved_per_path, uint64_t seed,
                       const sdmm_training_out* out, int64_t* n_out, int64_t* seg, int64_t* lost);

/* ---- The plugin's guiding model (SDMMVolumetricPathTracer) ----------------
 * volpath_sdmm.cpp:132-312, :411-507 on the device: the accelerator tree
 * (split_to_depth(split_depth) at creation, :398), one SDMM + EM state per
 * trained leaf, the leaves' training data and the per-iteration schedule.
 *   sdmm_guiding_push      Li's tail for a render pass (sdmm_push_training):
 *                          records appended to the leaves' data, own-leaf
 *                          positions to their stats (:894-902)
 *   sdmm_guiding_optimize  optimize() (:244-312): split every leaf by its stats
 *                          (split_leaf_recurse(threshold) under the leaf cap,
 *                          :253-259; a split leaf's data, stats and mixture go
 *                          to its new leaves -- jmm sntree.h:172-205), then per
 *                          leaf canBeOptimized (:140-149, with m_totalSpp of the
 *                          previous passes), initializeSDMMContext on first use
 *                          (K/8 positions = the leaf's first records, spatial
 *                          distance 3 hmax(diagonal) / (K/8), :132-138, :291),
 *                          2 EM iterations while iterations_run < 4 else 1
 *                          (:299-305) as ONE batched launch, the optimised
 *                          leaves' data cleared (:308-309); the trained leaves
 *                          are bound to the tree for the next pass.  spp: the
 *                          pass's samples per pixel (m_totalSpp += spp after).
 *   sdmm_guiding_iteration one pass of render()'s loop (:411-507): sdmm_li_render
 *                          (guided once a leaf is trained, :311-316), then
 *                          push + optimize when train (m_still_training).
 * Everything runs on the model's stream (= its tree's); calls return when
 * the host-side state is updated. */
typedef struct sdmm_guiding sdmm_guiding;
typedef struct {
    int K;                  /* components per leaf (16, SDMMProcess::NComponents) */
    int split_depth;        /* 2 */
    int split_threshold;    /* 4000 */
    int max_leaf_nodes;     /* 2048 */
    int saved_per_path;     /* 8 */
    float depth_prior;      /* 0.01 (sdmm-lib initialize is absent: jmm uniformHemisphereInit's) */
    uint64_t init_seed;     /* leaf v's hemisphere init seed = init_seed + v */
    int optimize_async;     /* optimizeAsync (volpath_sdmm.cpp:65, :180-242): one EM step per leaf (0.1 x
                               hmax(diagonal) at init) on the model's EM stream, overlapping the next pass;
                               renders use each leaf's conditioner, updated after the pass (sdmm_guiding_update) */
} sdmm_guiding_config;
typedef struct {
    int leaves;             /* leaf_nodes() after the split */
    int optimized;          /* leaves stepped this call */
    int64_t records;        /* pool records before the optimised leaves' were dropped */
} sdmm_guiding_stats;
void sdmm_guiding_config_default(sdmm_guiding_config* c);
int sdmm_guiding_create(const float tree_min[3], const float tree_max[3], const sdmm_guiding_config* cfg,
                        int device, sdmm_guiding** out);
void sdmm_guiding_destroy(sdmm_guiding* g);
sdmm_stree* sdmm_guiding_tree(sdmm_guiding* g);
int sdmm_guiding_node_mixtures(const sdmm_guiding* g, const sdmm_mix** out, int cap);
int sdmm_guiding_trained(const sdmm_guiding* g);
int sdmm_guiding_push(sdmm_guiding* g, const sdmm_path_vertices* v, uint64_t seed);
int sdmm_guiding_optimize(sdmm_guiding* g, int spp, sdmm_guiding_stats* out);
/* async: optimize_async_wait_and_update (:227-242) -- wait for the running EM,
 * copy each stepped leaf's mixture into its conditioner; no-op otherwise. */
int sdmm_guiding_update(sdmm_guiding* g);
int sdmm_guiding_iteration(sdmm_guiding* g, sdmm_scene* scene, const sdmm_li_params* p, uint64_t push_seed,
                           int train, float* image, float* image_sqr, sdmm_li_stats* li_stats,
                           sdmm_guiding_stats* out);

/* SDMMWorkResult::dumpIndividual (sdmm_wr.cpp:115-146): an RGB float OpenEXR
 * file (uncompressed scanlines, channels B G R, attributes spp / iteration
 * (int) and time (float) as Bitmap::setMetadata writes them) from HOST planes
 * rgb[3][height][width].  The plugin writes iteration%05i.exr (the pass's
 * mean) and iteration_sqr%05i.exr (its mean of squares) per render pass. */
int sdmm_write_exr(const char* path, int width, int height, const float* rgb, int spp, int iteration, float time);

/* The reader of what sdmm_write_exr writes (the reference reads its dumps with
 * pyexr: scripts/combine_renders.py:44-51): a single-part scanline file,
 * uncompressed, FLOAT channels among which R, G and B, listed in any order,
 * into HOST planes rgb[3][height][width] (R, G, B); rgb NULL: a size query.
 * *spp, *iteration, *time (each nullable) take the attributes of those names,
 * 0 / 0 / 0.0f where the file has none.  Anything else is SDMM_E_INVALID with
 * a message: a compression, a HALF or UINT channel, tiles, a missing channel,
 * a truncated file, a line offset or a data window pointing outside the file,
 * more than 2^26 pixels.  Every offset is checked before it is followed. */
int sdmm_read_exr(const char* path, int* width, int* height, float* rgb, int* spp, int* iteration, float* time);

/* ---- film: a run's passes combined by inverse variance, and its errors -----
 * The reference integrator composes no final image; its results come from
 * scripts/combine_renders.py and scripts/test_suite_utils.py run over the
 * dumped passes.  The film is that stage, fed straight from the planes
 * sdmm_li_render / sdmm_guiding_iteration write ("Film"; the
 * arithmetic: csrc/film.h).
 *
 * device >= 0: a device film; every image pointer is a device block of planes
 * [3][height * width] and work is enqueued on the call's hip_stream.  Calls on
 * one film must be ordered by the caller (one stream, or events).
 * device = -1: a host film; the same code on the CPU over host pointers,
 * hip_stream ignored, no HIP call: it runs on a machine without a GPU and its
 * results are bitwise the device film's (NaN payloads aside).
 *
 * Validation (SDMM_E_INVALID with a message): NULL handles and pointers, width
 * or height < 1 or more than 2^26 pixels, an unknown mode, first_iteration < 0,
 * spp < 2 (the variance divides by spp - 1). */
typedef struct sdmm_film sdmm_film;
enum {
    SDMM_FILM_VAR = 0,       /* 'var' (the default of combine_renders.py:167): weight = per-channel variance */
    SDMM_FILM_MAX_VAR = 1,   /* 'max_var': max(pixel variance, per-channel variance), NaN kept */
    SDMM_FILM_UNIFORM = 2    /* 'uniform': 1 / spp */
};
typedef struct {
    double pcv[3];               /* per_channel_variance (:220), an fp64 mean */
    double mean_pixel_variance;  /* var_data (:229), stats.json's mean_pixel_variance */
    int included;                /* iteration >= first_iteration (:230) */
} sdmm_film_stats;
typedef struct {
    double mrse, mape, smape;    /* test_suite_utils.py:148-155 under aggregate (:116-118) */
} sdmm_film_error;
/* first_iteration: the first pass that enters the estimate (the reference: 4). */
int sdmm_film_create(int width, int height, int mode, int first_iteration, int device, sdmm_film** out);
void sdmm_film_destroy(sdmm_film* f);
/* One pass (combine_renders.py:206-242): its variance statistics, and, when
 * included, final += image / w and recip += 1 / w.  image / image_sqr: the
 * pass's mean and mean of squares.  pass_stats NULL: a device film returns
 * with the work in flight (no host synchronisation); otherwise the stream is
 * synchronised and *pass_stats filled. */
int sdmm_film_add_pass(sdmm_film* f, const float* image, const float* image_sqr, int spp, int iteration,
                       void* hip_stream, sdmm_film_stats* pass_stats);
/* The history of pass statistics (host side; a device film synchronises the
 * stream of its last pass to fetch what is still in flight).  sdmm_film_passes:
 * the count, -1 for a NULL film. */
int sdmm_film_passes(const sdmm_film* f);
int sdmm_film_pass_stats(sdmm_film* f, int i, sdmm_film_stats* out);
/* final / recip (:246) into out[3][height * width]; SDMM_E_STATE before the
 * first included pass.  Asynchronous on hip_stream for a device film. */
int sdmm_film_resolve(sdmm_film* f, float* out, void* hip_stream);
/* MrSE, MAPE, SMAPE against ground_truth (:251-257): of `image`, or, image
 * NULL, of the current combined estimate (SDMM_E_STATE before the first
 * included pass) -- the reference's INDIVIDUAL and CUMULATIVE error types.
 * Synchronises hip_stream. */
int sdmm_film_errors(sdmm_film* f, const float* image, const float* ground_truth, void* hip_stream,
                     sdmm_film_error* out);
/* The clipped per-pixel variance of a pass (:213-219) into out[3][height *
 * width]; changes no film state.  Asynchronous on hip_stream for a device film. */
int sdmm_film_variance(const sdmm_film* f, const float* image, const float* image_sqr, int spp, float* out,
                       void* hip_stream);
/* Forget every pass (a device film synchronises the stream of its last pass). */
int sdmm_film_reset(sdmm_film* f);

const char* sdmm_last_error(void);
int sdmm_abi_version(void);

/* Library teardown (no reference counterpart: sdmm-lib holds no device state
 * outside its contexts).  Frees the per-(device, stream) scratch pool that
 * init / clone / k-means++ calls keep between calls.  Call only when no other
 * thread is inside the library; later calls regrow the pool on demand. */
int sdmm_release_cached_scratch(void);

#ifdef __cplusplus
}
#endif
#endif /* SDMM_GPU_H */
