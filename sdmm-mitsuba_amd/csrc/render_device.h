// render_device.h -- records shared by the device Li / training producer
// (render.hip) and their host launchers (render_api.cpp, sdmm_api.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mesh_bvh.h"
#include "envmap.h"
#include "texture.h"

namespace sdmm {

// ---- counter-based RNG (host + device; oracle/sdmm_oracle_train.c restates) ----
__host__ __device__ __forceinline__ uint64_t rng_mix(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// uniform in [0, 1): 24 random bits, exact in float
__host__ __device__ __forceinline__ float rng_uniform(uint64_t seed, uint64_t path, uint32_t stream, uint32_t dim) {
    const uint64_t k = rng_mix(rng_mix(seed ^ (path * 0xD1B54A32D192ED03ull)) + (((uint64_t)stream << 16) | dim));
    return (float)(uint32_t)(k >> 40) * (1.0f / 16777216.0f);
}
// streams: 0 camera; 1 + b bounce b (dims: 0-1 BSDF sample, 2 BSDF/guide
// choice, 3-5 guide sample, 6 roulette, 7 a rough dielectric's lobe choice; a
// smooth dielectric's lobe choice is dim 0, dim 1 -- the other half of the
// reference's nextSample2D -- stays unused);
// kJitterStream + d: vertex d's jitters
constexpr uint32_t kJitterStream = 1024;

constexpr int kVertexFields = 16;          // weight 3, throughput 3, pdf, point 6, normal 3

struct QuadDev {
    float p0[3], e1[3], e2[3];   // corner and edges (world)
    float n[3];                  // unit normal (flipNormals applied)
    float g1[3], g2[3];          // dual vectors: (p - p0).g1, (p - p0).g2 in [0, 1] on the quad
    int bsdf, emitter;           // emitter -1: none
};

// Per-BSDF parameters beside the diffuse reflectance (kBsdfParams floats per
// BSDF): [0] kind (0 diffuse, 1 smooth plastic, 2 rough conductor, 3 Phong, 4
// rough dielectric, 5 smooth dielectric, 6 smooth conductor).
// Plastic: [1..3] specular reflectance, [4] eta = intIOR / extIOR, [5] 1 /
// eta^2, [6] the internal diffuse Fresnel reflectance fdrInt, [7] the
// specular sampling weight sAvg / (dAvg + sAvg) (bsdfs/plastic.cpp:159-200).
// Rough conductor: [1..3] specular reflectance, [4] eta, [5] k (a gray
// conductor), [6] the Beckmann alpha, [7] unused (bsdfs/roughconductor.cpp).
// Phong: [1..3] specular reflectance, [4] exponent, [5] the specular sampling
// weight sAvg / (dAvg + sAvg), [6], [7] unused (bsdfs/phong.cpp:129-156).
// Rough dielectric: [1..3] specular reflectance, [4] eta = intIOR / extIOR,
// [5] 1 / eta, [6] the Beckmann alpha, [7] unused; its specularTransmittance
// in the BSDF's reflectance row (bsdfs/roughdielectric.cpp:213-241).
// Smooth dielectric: the rough one's layout without the alpha -- [1..3]
// specular reflectance, [4] eta, [5] 1 / eta, [6], [7] unused; its
// specularTransmittance in the reflectance row (bsdfs/dielectric.cpp).
// Smooth conductor: [1..3] specular reflectance, [4] eta, [5] k (gray), the
// rest unused (bsdfs/conductor.cpp).  Both are delta only (bsdf_smooth.h).
constexpr int kBsdfParams = 8;
constexpr int kBsdfDiffuse = 0;
constexpr int kBsdfPlastic = 1;
constexpr int kBsdfConductor = 2;
constexpr int kBsdfPhong = 3;
constexpr int kBsdfDielectric = 4;
constexpr int kBsdfSmoothDielectric = 5;
constexpr int kBsdfSmoothConductor = 6;

struct SceneDev {
    const QuadDev* quads;
    int n_quads;
    const float* refl;    // 3 per BSDF (plastic: its diffuseReflectance)
    const float* bpar;    // kBsdfParams per BSDF; null: every BSDF diffuse
    const float* lmodel;  // kLearnedStride per BSDF: [M, M SDMM4 records] (learned_bsdf.h); null: none
    const float* lmodel_nd;   // kLearnedNdStride per BSDF: [C, M, M records of learned_rec(C)]; null: none
    const float* rad;     // 3 per emitter
    float cam[12];        // camera-to-world 3x4 (row major)
    float tanx, aspect, near_clip;
    int width, height;
    float smin[3], snorm;
    int has_phong;        // some BSDF is Phong: the Li kernels' PHONG variants run
    int has_dielectric;   // some BSDF is a rough dielectric, or smooth (kinds 5, 6): their DIEL variants run
    // triangle mesh (mesh_bvh.h; primitive ids n_quads + i): null / 0 without one
    const BvhNode* nodes;
    const MeshTri* tris;      // leaf order
    const MeshHit* hits;      // by triangle index
    int n_tris;
    int has_mesh;         // the Li kernels' MESH variants run
    int mesh_brute;       // SDMM_MESH_BRUTE=1: the loop over all triangles instead of the BVH (A/B)
    // environment emitter (envmap.h): kind 0 without one; otherwise the camera
    // and shade kernels' ENV variants run
    EnvDev env;
    // 1 per BSDF wrapped in the single-child twosided adapter (twosided.cpp);
    // null: no BSDF is, and every kernel takes today's one-sided rule
    const int32_t* twosided;
};

// What only the NRM variants of the Li kernels read (a mesh with vertex
// normals, shading_normal.h): a record of its own, passed after every other
// kernel argument, so that SceneDev, PathsDev and the argument layout of the
// variants every other scene runs stay what they were.
struct NormalsDev {
    // the mesh's vertex normals by triangle index; null: none, every hit's
    // shading and geometric normal is its face normal
    const MeshShade* shade;
    // the current hit's shading and geometric normal, one plane a component:
    // written by the kernel that traced the ray (camera, shade), read by the
    // next bounce's kernels; null without vertex normals
    float *nsx, *nsy, *nsz;
    float *ngx, *ngy, *ngz;
    int strict;              // strictNormals of this render (sdmm_li_params.non_strict_normals == 0)
};

// the shading normal ns and the geometric normal ng of the hit of the ray (o,
// d) on primitive q, as sdmm_scene_shading reports them: a triangle with
// vertex normals through shading_normals, anything else its face normal twice
__host__ __device__ __forceinline__ void hit_normals(const SceneDev& S, const MeshShade* shade, int q,
                                                     const float o[3], const float d[3], float ns[3], float ng[3]) {
    if (q >= S.n_quads) {
        const int ti = q - S.n_quads;
        if (shade) {
            shading_normals(shade[ti], S.hits[ti].n, o, d, ns, ng);
            return;
        }
        for (int a = 0; a < 3; ++a) ns[a] = ng[a] = S.hits[ti].n[a];
        return;
    }
    for (int a = 0; a < 3; ++a) ns[a] = ng[a] = S.quads[q].n[a];
}

// What only the TEX variants of the Li kernels read (a scene whose BSDFs carry
// bitmap textures, texture.h): a record of its own, passed after every other
// kernel argument (after NormalsDev where both are), as NormalsDev is and for
// the same reason.
struct TexDev {
    const TextureDev* tex;       // the scene's textures (texels: TexTexel on the device)
    const int32_t* bsdf_tex;     // per BSDF: its reflectance's texture, -1 none; null: no BSDF is textured
    const MeshUV* mesh_uv;       // by triangle index; null without a mesh (or with neither mesh_uvs nor textures)
    // the current hit's effective reflectance (the texture's value at the
    // hit's uv, or the BSDF's row), one plane a channel: written by the kernel
    // that traced the ray (camera, shade), read by the next bounce's kernels;
    // null without textures
    float *rr, *rg, *rb;
};

// the effective reflectance of BSDF b at a hit with texture coordinates uv:
// its texture's value, or its row
template <bool RGBA>
__host__ __device__ __forceinline__ void hit_reflectance(const float* refl, const TextureDev* tex,
                                                         const int32_t* bsdf_tex, int b, const float uv[2],
                                                         float rgb[3]) {
    const int ti = bsdf_tex ? bsdf_tex[b] : -1;
    if (ti >= 0) {
        tex_eval<RGBA>(tex[ti], uv, rgb);
        return;
    }
    for (int ch = 0; ch < 3; ++ch) rgb[ch] = refl[3 * b + ch];
}

// hit_normals and hit_uv (texture.h) of one hit together: on a triangle with
// vertex normals the test on the winner runs once and serves both
__host__ __device__ __forceinline__ void hit_normals_uv(const SceneDev& S, const MeshShade* shade,
                                                        const MeshUV* mesh_uv, int q, const float o[3],
                                                        const float d[3], float ns[3], float ng[3], float uv[2]) {
    if (q >= S.n_quads && shade) {
        const int ti = q - S.n_quads;
        float t, u = 0.0f, v = 0.0f;
        const bool hit = tri_intersect_uv(shade[ti].tri, o, d, &t, &u, &v);
        shading_normals_at(shade[ti], S.hits[ti].n, hit, u, v, ns, ng);
        uv[0] = uv[1] = 0.0f;
        if (hit) tri_uv(mesh_uv[ti], u, v, uv);
        return;
    }
    hit_normals(S, nullptr, q, o, d, ns, ng);
    hit_uv(S.quads, S.n_quads, mesh_uv, q, o, d, uv);
}

// a hit from behind (cos_i = wi . n < 0) on a two-sided BSDF: the bounce runs
// in (s, t, -n) of Frame(n) (wi.z *= -1 ... wo.z *= -1, twosided.cpp:111-137,
// :191-213) and the saved vertex carries -n (sdmm_proc.cpp:765-767)
__device__ __forceinline__ bool twosided_back(const SceneDev& S, int bsdf, float cos_i) {
    return S.twosided && S.twosided[bsdf] != 0 && cos_i < 0.0f;
}

// closest quad with t in (mint, maxt), the lowest id on equal t (strict <);
// -1: none, *t_hit = maxt then.  Host + device, bitwise alike.
__host__ __device__ __forceinline__ int quads_closest(const QuadDev* quads, int n_quads, const float o[3],
                                                      const float d[3], float mint, float maxt, float& t_hit) {
#pragma clang fp contract(off)
    int best = -1;
    float tb = maxt;
    for (int q = 0; q < n_quads; ++q) {
        const QuadDev& Q = quads[q];
        const float denom = d[0] * Q.n[0] + d[1] * Q.n[1] + d[2] * Q.n[2];
        if (denom == 0.0f) continue;
        const float r0[3] = {Q.p0[0] - o[0], Q.p0[1] - o[1], Q.p0[2] - o[2]};
        const float t = (r0[0] * Q.n[0] + r0[1] * Q.n[1] + r0[2] * Q.n[2]) / denom;
        if (!(t > mint && t < tb)) continue;
        const float r[3] = {o[0] + t * d[0] - Q.p0[0], o[1] + t * d[1] - Q.p0[1], o[2] + t * d[2] - Q.p0[2]};
        const float a = r[0] * Q.g1[0] + r[1] * Q.g1[1] + r[2] * Q.g1[2];
        const float b = r[0] * Q.g2[0] + r[1] * Q.g2[1] + r[2] * Q.g2[2];
        if (a < 0.0f || a > 1.0f || b < 0.0f || b > 1.0f) continue;
        tb = t;
        best = q;
    }
    t_hit = tb;
    return best;
}

struct PathsDev {
    float *px, *py, *pz;     // current hit point
    float *dx, *dy, *dz;     // direction of the ray that reached it
    float *tr, *tg, *tb;     // throughput
    float *lr, *lg, *lb;     // Li
    int* depth;              // rRec.depth; -1 once the path has ended
    int* quad;               // hit primitive (a quad, or n_quads + triangle)
    int* nv;                 // saved vertices
    int* nray;               // traced bounce rays (a delta bounce saves no vertex)
    float* rec;              // vertex records: rec[(f * V + v) * P + p]
    int V;
    int64_t P;
    float* eta;              // the path's relative index (sdmm_proc.cpp:788); null without DIEL kernels
};

struct QueryDev {
    float *c0, *c1, *c2;     // condition
    float *u0, *u1, *u2;     // guide sample
    float *b0, *b1, *b2;     // BSDF direction (world)
    uint8_t* mode;           // 1: BSDF chosen (pdf query), 0: guide sample
    float *d0, *d1, *d2;     // wavefront outputs (compact: query j = path idx[j])
    float* pdf;
    int32_t* comp;
    // compaction of the live guided queries: flag per path, the selected
    // path ids, each path's compact slot (-1: no query), compact inputs
    uint8_t* live;
    int32_t* idx;
    int32_t* slot;
    float *k_c0, *k_c1, *k_c2, *k_u0, *k_u1, *k_u2, *k_b0, *k_b1, *k_b2;
    uint8_t* k_mode;
    // product sampling (sampleProduct): the BSDF/guide draw per path (the
    // wavefront decides with the query's own h), and per compact query the
    // shading frame (row-major, columns s t n), the material and h out
    float* ch;
    float* k_ch;
    float* k_F[9];
    int32_t* k_mat;
    float* hq;
    // the loop head's BSDF sample for the shade kernel (non-diffuse BSDFs):
    // sampled lobe delta (1) or smooth (0), its weight (RGB) and pdf
    uint8_t* bdelta;
    float *bw0, *bw1, *bw2, *bpdf;
    float* beta;             // a dielectric's sample: the index it crossed (bRec.eta); null without DIEL kernels
    // product with a rough conductor's, a Phong BSDF's or a rough
    // dielectric's learned model:
    // compact query j's lobes (weights, local means, covariances) at row
    // lrow0 + j of the render's extended learned-BSDF table (lM lobes a row);
    // lw null: no such material
    float *lw, *lm, *lc;
    int lrow0, lM;
};

}  // namespace sdmm
