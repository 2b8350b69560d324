// render.hip -- the guided path tracer's device side: SDMMRenderer::Li
// (sdmm_proc.cpp:592-968) as a wavefront over an analytic quad scene, and the
// training-data producer of its tail (push_back_data + jittered neighbour
// routing, :876-965).
//
// One path per thread, path state in SoA planes in HBM.  A bounce is three
// launches on one stream:
//   li_query_kernel   the loop head for every live path (:649-691): depth cap,
//                     condition c = (p - scene_min) / spatial_norm
//                     (createCondition :263-273), the BSDF direction and the
//                     plugin's BSDF/guide choice (h = 0.5, :383-392);
//   the guided wavefront (guide.hip, sdmm_guide_pdf_wavefront): the leaf's
//                     conditional built once per query, then a GMM sample or
//                     the gmmPdf of the BSDF direction (:368-421, :510-590);
//   li_shade_kernel   the rest of sampleSurface (:392-507) and of the loop
//                     body (:759-871): BSDF weight / mixture pdf, throughput,
//                     the next ray, the emitter it hits, recordRadiance and the
//                     saved vertex (:815-846), Russian roulette.
// The camera kernel starts the paths (first hit, its emission: :641-677); the
// film kernel averages each pixel's samples in sample order (box filter).
//
// Scene: parallelograms (Mitsuba rectangles; a cube is six) and an optional
// triangle mesh (its BVH walked by the MESH variants of the camera and shade
// kernels: mesh_bvh.h; face normals, or with sdmm_scene_desc.mesh_normals the
// interpolated shading normal beside the geometric one, shading_normal.h, and
// the strictNormals tests: the NRM variants), diffuse BSDFs
// (diffuse.cpp: cosine-hemisphere sampling, f = rho / pi) and smooth plastic
// (plastic.cpp: a delta specular lobe with the dielectric Fresnel reflectance
// over a diffuse base, the lobe chosen by Fresnel-weighted probability), rough
// conductors, Phong BSDFs (bsdf_phong.h) and rough dielectrics
// (bsdf_roughdielectric.h: two-sided, transmitting), smooth dielectrics and
// smooth conductors (bsdf_smooth.h: delta only -- such a bounce queries no
// guide and saves no vertex), each non-transmitting kind optionally under the
// single-child twosided adapter (twosided.cpp, SceneDev::twosided: a hit from
// behind runs the nested BSDF in (s, t, -n) of Frame(n), saves -n with its
// vertex and hands the product F = [s t -n]; the two-child form and two-sided
// emitters are not done), a bitmap texture in place of a diffuse, plastic or
// Phong BSDF's reflectance row (texture.h: the TEX variants),
// one-sided area emitters (area.cpp: Le = radiance on the normal side) and an
// optional environment emitter (envmap.h: constant or lat-long map, seen by
// every ray that leaves the scene).  No NEE (the plugin's
// NEE block is compiled out, :700-734; emitterPdf = 0, MIS weight 1, :811-816).
//
// Random numbers: counter-based (rng_uniform below), one fixed slot per
// (path, stream, dimension) -- a path's outcome does not depend on which other
// paths run, nor on the order the reference's sampler would consume numbers;
// the reference's Mitsuba sampler itself is not reproducible here.
#include "sdmm_device.h"
#include "render_device.h"
#include "render_launch.h"
#include "learned_bsdf.h"
#include "bsdf_phong.h"
#include "bsdf_beckmann.h"
#include "bsdf_roughdielectric.h"
#include "bsdf_smooth.h"

#include <hipcub/hipcub.hpp>

#pragma clang fp contract(off)

namespace sdmm {

// RNG, scene / path / query records: render_device.h
constexpr float kEpsilon = 1e-4f;          // Mitsuba single-precision Epsilon (ray mint)
constexpr float kInvPi = 0.31830988618379067154f;

// dot3, normalize3 and the Beckmann distribution (beckmann_d, beckmann_g1,
// beckmann_sample_all): bsdf_beckmann.h

// closest hit with t in (mint, maxt); -1: none.  Quads by their loop
// (quads_closest, render_device.h); MESH: then the triangles through the BVH
// (mesh_bvh.h), its stack in LDS as [level][thread] -- stack points at this
// thread's column, 256 apart.  Primitive id: a quad, or n_quads + triangle.
struct LdsStack {
    int* col;
    __device__ __forceinline__ void push(int level, int node) { col[level * 256] = node; }
    __device__ __forceinline__ int pop(int level) const { return col[level * 256]; }
};
template <bool MESH>
__device__ __forceinline__ int intersect(const SceneDev& S, const float o[3], const float d[3], float mint,
                                         float maxt, float& t_hit, int* stack) {
    int best = quads_closest(S.quads, S.n_quads, o, d, mint, maxt, t_hit);
    if constexpr (MESH) {
        if (S.mesh_brute) {
            mesh_brute(S.tris, S.n_tris, S.n_quads, o, d, mint, maxt, best, t_hit);
        } else {
            LdsStack st{stack};
            bvh_closest(S.nodes, S.tris, S.n_quads, o, d, mint, maxt, best, t_hit, st);
        }
    }
    return best;
}
// the hit primitive's normal, BSDF and emitter: a quad's fields, or (MESH, q
// >= n_quads) the triangle's hit record
template <bool MESH>
__device__ __forceinline__ const float* prim_n(const SceneDev& S, int q) {
    if constexpr (MESH)
        if (q >= S.n_quads) return S.hits[q - S.n_quads].n;
    return S.quads[q].n;
}
template <bool MESH>
__device__ __forceinline__ int prim_bsdf(const SceneDev& S, int q) {
    if constexpr (MESH)
        if (q >= S.n_quads) return S.hits[q - S.n_quads].bsdf;
    return S.quads[q].bsdf;
}
template <bool MESH>
__device__ __forceinline__ int prim_emitter(const SceneDev& S, int q) {
    if constexpr (MESH)
        if (q >= S.n_quads) return S.hits[q - S.n_quads].emitter;
    return S.quads[q].emitter;
}
// NRM: the Li kernels' variants for a mesh with vertex normals (MESH only).
// They take the normals' record as one more, last argument -- the parameter
// pack Nrm = {NormalsDev}; the variants every other scene runs have an empty
// pack, so their arguments are what they always were.
// TEX: the variants for a scene whose BSDFs carry bitmap textures (texture.h),
// the camera, query and shade kernels': TexDev rides in the same pack, after
// NormalsDev where both are -- Nrm = {}, {NormalsDev}, {TexDev} or {NormalsDev,
// TexDev}.  pack_has<T>: the pack holds a T; pack_get<T>: it.
template <class T, class... X>
constexpr bool pack_has = (std::is_same_v<T, X> || ...);
template <class T, class A, class... X>
__device__ __forceinline__ T pack_get(A a, X... x) {
    if constexpr (std::is_same_v<T, A>) return a;
    else return pack_get<T>(x...);
}
template <class... X>
__device__ __forceinline__ NormalsDev nrm_arg(X... x) { return pack_get<NormalsDev>(x...); }
template <class... X>
__device__ __forceinline__ TexDev tex_arg(X... x) { return pack_get<TexDev>(x...); }
// The current hit's shading normal: NRM from the path's planes, where the
// kernel that traced the ray left it -- otherwise the primitive's face normal,
// fetched by id as ever.  buf: the caller's three floats (unused without NRM).
template <bool MESH, class... Nrm>
__device__ __forceinline__ const float* path_ns(const SceneDev& S, int64_t i, int q, float buf[3], Nrm... nrm) {
    if constexpr (pack_has<NormalsDev, Nrm...>) {
        const NormalsDev N = nrm_arg(nrm...);
        buf[0] = N.nsx[i]; buf[1] = N.nsy[i]; buf[2] = N.nsz[i];
        return buf;
    } else {
        return prim_n<MESH>(S, q);
    }
}
__device__ __forceinline__ void store_normals(const NormalsDev& N, int64_t i, const float ns[3], const float ng[3]) {
    N.nsx[i] = ns[0]; N.nsy[i] = ns[1]; N.nsz[i] = ns[2];
    N.ngx[i] = ng[0]; N.ngy[i] = ng[1]; N.ngz[i] = ng[2];
}
// The current hit's effective reflectance: TEX from the path's planes, where
// the kernel that traced the ray left it (the texture's value at the hit, or
// the row of an untextured BSDF) -- otherwise BSDF qb's row, as ever.
template <class... Nrm>
__device__ __forceinline__ const float* path_rho(const SceneDev& S, int64_t i, int qb, float buf[3], Nrm... nrm) {
    if constexpr (pack_has<TexDev, Nrm...>) {
        const TexDev T = tex_arg(nrm...);
        buf[0] = T.rr[i]; buf[1] = T.rg[i]; buf[2] = T.rb[i];
        return buf;
    } else {
        return S.refl + 3 * qb;
    }
}
// The kernel that traced a ray (camera, shade) leaves the hit's effective
// reflectance in the path's planes: BSDF qb's texture at the hit's uv, or its
// row -- one lookup (four texels at most) per hit, coalesced reads afterwards.
__device__ __forceinline__ void store_reflectance(const SceneDev& S, const TexDev& T, int64_t i, int qb,
                                                  const float uv[2]) {
    float rgb[3];
    hit_reflectance<true>(S.refl, T.tex, T.bsdf_tex, qb, uv, rgb);
    T.rr[i] = rgb[0]; T.rg[i] = rgb[1]; T.rb[i] = rgb[2];
}
// the MESH kernels' traversal stack: kBvhStack levels x 256 threads of LDS
#define LI_MESH_STACK(stack)                              \
    int* stack = nullptr;                                 \
    if constexpr (MESH) {                                 \
        __shared__ int bvh_lds[kBvhStack * 256];          \
        stack = bvh_lds + threadIdx.x;                    \
    }

// Frame(n) (frame_of) and warp::squareToCosineHemisphere (cosine_hemisphere):
// bsdf_phong.h

// fresnelDielectricExt (libcore/util.cpp:651-681): the unpolarised
// reflectance at cos(theta_i) for the relative index eta
__device__ __forceinline__ float fresnel_dielectric(float cos_i, float eta) {
    if (eta == 1.0f) return 0.0f;
    const float scale = cos_i > 0.0f ? 1.0f / eta : eta;
    const float ct2 = 1.0f - (1.0f - cos_i * cos_i) * (scale * scale);
    if (ct2 <= 0.0f) return 1.0f;
    const float ci = fabsf(cos_i), ct = sqrtf(ct2);
    const float rs = (ci - eta * ct) / (ci + eta * ct);
    const float rp = (eta * ci - ct) / (eta * ci + ct);
    return 0.5f * (rs * rs + rp * rp);
}

// SmoothPlastic's specular sampling probability (plastic.cpp:339-342)
__device__ __forceinline__ float plastic_prob_specular(float Fi, float ssw) {
    // 0 / 0 (no specular weight at a total reflection, or weight 1 with Fi =
    // 0) is 0 here, NaN in plastic.cpp:339-342: both lobes then carry no
    // energy along that direction, and a NaN would only poison the sample
    const float num = Fi * ssw, den = num + (1.0f - Fi) * (1.0f - ssw);
    return den == 0.0f ? 0.0f : num / den;
}

// ---------------------------------------------------------------------------
// Rough conductor (bsdfs/roughconductor.cpp:296-470 over microfacet.h): the
// Beckmann distribution with isotropic alpha, sampleVisible = false (sampleAll
// / pdfAll, microfacet.h:287-407 -- a documented choice of the plugin), a gray
// conductor (eta, k equal over the channels; fresnelConductorExact's Spectrum
// form, libcore/util.cpp:739-761) times the specular reflectance.  The
// distribution itself: bsdf_beckmann.h.

// fresnel_conductor: bsdf_smooth.h (shared with the smooth conductor)

// RoughConductor::sample(bRec, pdf, sample) (roughconductor.cpp:414-462) in the
// local frame, wi.z > 0: wo, the weight F * (D G (wi.m) / (pdf cos)) and the
// solid-angle pdf; false: the sample is void (weight 0)
__device__ __forceinline__ bool conductor_sample(const float wi[3], const float* bp, float u0, float u1,
                                                 float wo[3], float bw[3], float* pdf) {
    const float alpha = bp[6];
    float m[3];
    const float mpdf = beckmann_sample_all(alpha, u0, u1, m);
    *pdf = 0.0f;
    bw[0] = bw[1] = bw[2] = 0.0f;
    wo[0] = 0.0f; wo[1] = 0.0f; wo[2] = 1.0f;
    if (mpdf == 0.0f) return false;
    const float dm = dot3(wi, m);
    for (int a = 0; a < 3; ++a) wo[a] = 2.0f * dm * m[a] - wi[a];   // reflect
    if (wo[2] <= 0.0f) return false;
    const float fr = fresnel_conductor<float>(dm, bp[4], bp[5]);
    const float g = beckmann_g1(wi, m, alpha) * beckmann_g1(wo, m, alpha);
    const float weight = beckmann_d(m, alpha) * g * dm / (mpdf * wi[2]);
    for (int ch = 0; ch < 3; ++ch) bw[ch] = fr * bp[1 + ch] * weight;
    *pdf = mpdf / (4.0f * dot3(wo, m));
    return true;
}

// RoughConductor::eval (ESolidAngle, :302-339) and pdf (:341-366) in the local
// frame
__device__ __forceinline__ float conductor_eval_pdf(const float wi[3], const float wo[3], const float* bp,
                                                    float f[3]) {
    f[0] = f[1] = f[2] = 0.0f;
    if (wi[2] <= 0.0f || wo[2] <= 0.0f) return 0.0f;
    const float alpha = bp[6];
    const float hs[3] = {wo[0] + wi[0], wo[1] + wi[1], wo[2] + wi[2]};
    float H[3];
    normalize3(hs, H);
    const float D = beckmann_d(H, alpha);
    if (D != 0.0f) {
        const float fr = fresnel_conductor<float>(dot3(wi, H), bp[4], bp[5]);
        const float G = beckmann_g1(wi, H, alpha) * beckmann_g1(wo, H, alpha);
        const float model = D * G / (4.0f * wi[2]);
        for (int ch = 0; ch < 3; ++ch) f[ch] = fr * bp[1 + ch] * model;
    }
    return D * H[2] / (4.0f * fabsf(dot3(wo, H)));
}

__device__ __forceinline__ float& vrec(const PathsDev& P, int f, int v, int64_t p) {
    return P.rec[((int64_t)f * P.V + v) * P.P + p];
}

// recordRadiance (:628-637): every saved vertex's weight gets the radiance
// divided by its throughput and sampling pdf (Vertex::record, :615-621)
__device__ __forceinline__ void record_radiance(const PathsDev& P, int64_t p, int nv, const float rad[3]) {
    for (int v = 0; v < nv; ++v) {
        const float pdf = vrec(P, 6, v, p);
        for (int ch = 0; ch < 3; ++ch) {
            const float thr = vrec(P, 3 + ch, v, p);
            if (thr > kEpsilon) vrec(P, ch, v, p) += rad[ch] / (thr * pdf);
        }
    }
}

// ---------------------------------------------------------------------------
// camera rays: pixel = path / spp (box filter, uniform jitter), Mitsuba's
// perspective mapping (fov along x): local d = ((1 - 2 sx) tan, (1 - 2 sy) tan / aspect, 1)
// ENV: the variant for a scene with an environment emitter (envmap.h): a ray
// that hits nothing returns evalEnvironment (sdmm_proc.cpp:659-671); the other
// scenes' kernels do not carry the lookup and keep their registers.
// NRM: the variant for a mesh with vertex normals (shading_normal.h): the hit's
// ns / ng are worked out here, once, and left in the path's planes; emission
// is seen on the shading normal's side (dot(its.shFrame.n, d) <= 0 gives 0,
// emitters/area.cpp:105).
// TEX: the variant for a scene with textured BSDFs (texture.h): the hit's uv
// and its BSDF's effective reflectance are worked out here, once, and left in
// the path's planes.
template <bool MESH, bool ENV, class... Nrm>
__global__ void __launch_bounds__(256)
li_camera_kernel(SceneDev S, PathsDev P, int64_t path0, int spp, uint64_t seed, Nrm... nrm) {
    constexpr bool NRM = pack_has<NormalsDev, Nrm...>, TEX = pack_has<TexDev, Nrm...>;
    static_assert(!NRM || MESH, "NRM: a MESH variant");
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.P) return;
    LI_MESH_STACK(stack)
    const int64_t gp = path0 + i;
    const int64_t pix = gp / spp;
    const int px = (int)(pix % S.width), py = (int)(pix / S.width);
    const float sx = ((float)px + rng_uniform(seed, (uint64_t)gp, 0, 0)) / (float)S.width;
    const float sy = ((float)py + rng_uniform(seed, (uint64_t)gp, 0, 1)) / (float)S.height;
    float l[3] = {(1.0f - 2.0f * sx) * S.tanx, (1.0f - 2.0f * sy) * S.tanx / S.aspect, 1.0f};
    const float inv = 1.0f / sqrtf(dot3(l, l));
    for (int a = 0; a < 3; ++a) l[a] *= inv;
    float d[3], o[3];
    for (int r = 0; r < 3; ++r) {
        d[r] = S.cam[4 * r] * l[0] + S.cam[4 * r + 1] * l[1] + S.cam[4 * r + 2] * l[2];
        o[r] = S.cam[4 * r + 3];
    }
    const float dn = 1.0f / sqrtf(dot3(d, d));
    for (int a = 0; a < 3; ++a) d[a] *= dn;
    float t;
    const int q = intersect<MESH>(S, o, d, S.near_clip / l[2], INFINITY, t, stack);
    P.tr[i] = 1.0f; P.tg[i] = 1.0f; P.tb[i] = 1.0f;
    P.nv[i] = 0;
    P.nray[i] = 0;
    P.dx[i] = d[0]; P.dy[i] = d[1]; P.dz[i] = d[2];
    float L[3] = {0.0f, 0.0f, 0.0f};
    if (q >= 0) {
        float hns[3], hng[3];
        const float* qn;
        if constexpr (NRM) {
            if constexpr (TEX) {
                // (the triangle test on the winner runs once for both)
                float uv[2];
                hit_normals_uv(S, nrm_arg(nrm...).shade, tex_arg(nrm...).mesh_uv, q, o, d, hns, hng, uv);
                store_reflectance(S, tex_arg(nrm...), i, prim_bsdf<MESH>(S, q), uv);
            } else {
                hit_normals(S, nrm_arg(nrm...).shade, q, o, d, hns, hng);
            }
            store_normals(nrm_arg(nrm...), i, hns, hng);
            qn = hns;
        } else {
            if constexpr (TEX) {
                float uv[2];
                hit_uv(S.quads, S.n_quads, tex_arg(nrm...).mesh_uv, q, o, d, uv);
                store_reflectance(S, tex_arg(nrm...), i, prim_bsdf<MESH>(S, q), uv);
            }
            qn = prim_n<MESH>(S, q);
        }
        const int qe = prim_emitter<MESH>(S, q);
        P.px[i] = o[0] + t * d[0]; P.py[i] = o[1] + t * d[1]; P.pz[i] = o[2] + t * d[2];
        // emission seen directly (:674-677), before any vertex exists
        if (qe >= 0 && -dot3(d, qn) > 0.0f)
            for (int ch = 0; ch < 3; ++ch) L[ch] = S.rad[3 * qe + ch];
    }
    // no hit: the environment seen directly (:659-671; throughput 1, no vertex yet)
    if constexpr (ENV)
        if (q < 0) env_eval<true>(S.env, d, L);
    P.lr[i] = L[0]; P.lg[i] = L[1]; P.lb[i] = L[2];
    P.quad[i] = q;
    P.depth[i] = q >= 0 ? 1 : -1;   // no hit: the path ends (with the environment's radiance, if any)
}

// ---------------------------------------------------------------------------
// Loop head of bounce b for every live path.  guided: the tree holds trained
// leaves (m_iteration != 0, :311-316); otherwise every query is BSDF only.
// PHONG: the variant for a scene with Phong BSDFs (the three Li kernels carry
// Phong's code only there, so the other scenes' kernels keep their registers).
// DIEL: likewise for a scene with rough dielectrics (bsdf_roughdielectric.h):
// two-sided hits, the transmitted lobe and the path's relative index eta; and
// for the delta-only BSDFs of bsdf_smooth.h (kinds 5 and 6), whose bounce takes
// the sampled direction without a guide query (sdmm_proc.cpp:297-302).
// NRM: with vertex normals everything here runs on the hit's shading normal,
// and strictNormals' first test ends the path whose wi lies on different sides
// of the two normals ((wi . ng)(wi . ns) < 0, sdmm_proc.cpp:688-691).
// TEX: the reflectance of kinds 0, 1 and 3 is the hit's own, from the path's
// planes; the zero-reflectance rule then holds per hit.
template <bool PHONG, bool DIEL, bool MESH, class... Nrm>
__global__ void __launch_bounds__(256)
li_query_kernel(SceneDev S, PathsDev P, QueryDev Q, int64_t path0, int bounce, int max_depth, int guided,
                float h, uint64_t seed, Nrm... nrm) {
    constexpr bool NRM = pack_has<NormalsDev, Nrm...>, TEX = pack_has<TexDev, Nrm...>;
    static_assert(!NRM || MESH, "NRM: a MESH variant");
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.P) return;
    if (DIEL && bounce == 0) P.eta[i] = 1.0f;   // Float eta = 1.0f (sdmm_proc.cpp:604)
    int depth = P.depth[i];
    bool live = depth >= 0;
    if (live && max_depth >= 0 && depth >= max_depth) live = false;   // :684-685
    int q = live ? P.quad[i] : -1;
    float n[3] = {0, 0, 0}, wi[3] = {0, 0, 0};
    bool pure_delta = false;            // a kind-5 or kind-6 hit (DIEL)
    bool back = false;                  // a two-sided BSDF met from behind
    float rbuf[3];                      // (TEX: the hit's reflectance)
    if (live) {
        const float* qn = prim_n<MESH>(S, q);
        const int qb = prim_bsdf<MESH>(S, q);
        n[0] = qn[0]; n[1] = qn[1]; n[2] = qn[2];
        wi[0] = -P.dx[i]; wi[1] = -P.dy[i]; wi[2] = -P.dz[i];
        if constexpr (NRM) {
            // (the shading normal in the face normal's place, and strictNormals' first test)
            const NormalsDev N = nrm_arg(nrm...);
            n[0] = N.nsx[i]; n[1] = N.nsy[i]; n[2] = N.nsz[i];
            if (N.strict) {
                const float ng[3] = {N.ngx[i], N.ngy[i], N.ngz[i]};
                if (dot3(wi, ng) * dot3(wi, n) < 0.0f) live = false;
            }
        }
        // (TEX: the hit's own reflectance, so a hit on a black texel ends the
        // path here as bsdfWeight.isZero() does in the reference)
        const float* rho = path_rho(S, i, qb, rbuf, nrm...);
        const float* bp = S.bpar ? S.bpar + kBsdfParams * qb : nullptr;
        const int kind = bp ? (int)bp[0] : kBsdfDiffuse;
        const bool zero_spec = kind == kBsdfDiffuse || (bp[1] == 0.0f && bp[2] == 0.0f && bp[3] == 0.0f);
        const bool zero_diff = kind == kBsdfConductor || (DIEL && kind == kBsdfSmoothConductor) ||
                               (rho[0] == 0.0f && rho[1] == 0.0f && rho[2] == 0.0f);
        // no reflection from the back side or with zero reflectances (the
        // light's BSDF): sample and eval are 0, the path ends (:772-774)
        // (a rough dielectric is live from either side: it dies only at
        // wi . n == 0 or with both its reflectance and transmittance zero; so
        // is a smooth one, a smooth conductor is one-sided; the twosided
        // adapter makes its BSDF live from behind too: back)
        const float cos_i = dot3(wi, n);
        back = twosided_back(S, qb, cos_i);
        const bool side = DIEL && (kind == kBsdfDielectric || kind == kBsdfSmoothDielectric)
                              ? (cos_i > 0.0f || cos_i < 0.0f)
                              : (cos_i > 0.0f || back);
        if (!side || (zero_diff && zero_spec)) live = false;
        if (DIEL) pure_delta = kind == kBsdfSmoothDielectric || kind == kBsdfSmoothConductor;
    }
    // (a pure-delta bounce sends no query to the guided wavefront, :297-302)
    Q.live[i] = (uint8_t)((live && guided && !pure_delta) ? 1 : 0);
    Q.slot[i] = -1;
    if (!live) {
        P.depth[i] = -1;
        return;
    }
    const uint64_t gp = (uint64_t)(path0 + i);
    const uint32_t stream = 1u + (uint32_t)bounce;
    const float p[3] = {P.px[i], P.py[i], P.pz[i]};
    Q.c0[i] = (p[0] - S.smin[0]) / S.snorm;
    Q.c1[i] = (p[1] - S.smin[1]) / S.snorm;
    Q.c2[i] = (p[2] - S.smin[2]) / S.snorm;
    float s[3], t[3], w[3];
    frame_of(n, s, t);
    // a back hit: the frame (s, t, -n) -- Frame(n)'s tangents kept, so local
    // wi is (wi.s, wi.t, -(wi.n)) and w goes to world as s w0 + t w1 - n w2
    if (back)
        for (int a = 0; a < 3; ++a) n[a] = -n[a];
    const float* bp = S.bpar ? S.bpar + kBsdfParams * prim_bsdf<MESH>(S, q) : nullptr;
    uint8_t delta = 0;
    if (bp && bp[0] == (float)kBsdfPlastic) {
        // SmoothPlastic::sample(bRec, pdf, sample) (plastic.cpp:378-420): the
        // delta mirror lobe with probability probSpecular, else the cosine
        // hemisphere on the rescaled first coordinate; weight and pdf for the
        // shade kernel (a mixture bounce keeps the sampled lobe, :392-407)
        const float* rho = path_rho(S, i, prim_bsdf<MESH>(S, q), rbuf, nrm...);
        const float wl[3] = {dot3(wi, s), dot3(wi, t), dot3(wi, n)};   // Frame::toLocal
        const float Fi = fresnel_dielectric(wl[2], bp[4]);
        const float ps = plastic_prob_specular(Fi, bp[7]);
        const float u0 = rng_uniform(seed, gp, stream, 0), u1 = rng_uniform(seed, gp, stream, 1);
        if (u0 < ps) {
            delta = 1;
            w[0] = -wl[0]; w[1] = -wl[1]; w[2] = wl[2];
            // Spectrum * Fi / probSpecular (TSpectrum::operator/: times the reciprocal)
            const float rs = 1.0f / ps;
            Q.bw0[i] = bp[1] * Fi * rs; Q.bw1[i] = bp[2] * Fi * rs; Q.bw2[i] = bp[3] * Fi * rs;
            Q.bpdf[i] = ps;
        } else {
            cosine_hemisphere((u0 - ps) / (1.0f - ps), u1, w);
            const float Fo = fresnel_dielectric(w[2], bp[4]);
            // diff /= 1 - fdrInt; diff * (invEta2 (1 - Fi) (1 - Fo) / (1 - probSpecular))
            const float rd = 1.0f / (1.0f - bp[6]);
            const float k = bp[5] * (1.0f - Fi) * (1.0f - Fo) / (1.0f - ps);
            Q.bw0[i] = rho[0] * rd * k;
            Q.bw1[i] = rho[1] * rd * k;
            Q.bw2[i] = rho[2] * rd * k;
            Q.bpdf[i] = (1.0f - ps) * (kInvPi * w[2]);
        }
    } else if (bp && bp[0] == (float)kBsdfConductor) {
        // RoughConductor::sample (roughconductor.cpp:414-462); a void sample
        // has weight 0 (the path ends if the BSDF direction is taken)
        const float wl[3] = {dot3(wi, s), dot3(wi, t), dot3(wi, n)};
        float bw[3], bpdf;
        conductor_sample(wl, bp, rng_uniform(seed, gp, stream, 0), rng_uniform(seed, gp, stream, 1), w, bw, &bpdf);
        Q.bw0[i] = bw[0]; Q.bw1[i] = bw[1]; Q.bw2[i] = bw[2];
        Q.bpdf[i] = bpdf;
    } else if (PHONG && bp && bp[0] == (float)kBsdfPhong) {
        // Phong::sample (phong.cpp:232-289); a void sample has weight 0
        const float* rho = path_rho(S, i, prim_bsdf<MESH>(S, q), rbuf, nrm...);
        const float wl[3] = {dot3(wi, s), dot3(wi, t), dot3(wi, n)};
        float bw[3], bpdf;
        phong_sample(wl, bp, rho, rng_uniform(seed, gp, stream, 0), rng_uniform(seed, gp, stream, 1), w, bw, &bpdf);
        Q.bw0[i] = bw[0]; Q.bw1[i] = bw[1]; Q.bw2[i] = bw[2];
        Q.bpdf[i] = bpdf;
    } else if (DIEL && bp && bp[0] == (float)kBsdfDielectric) {
        // RoughDielectric::sample (roughdielectric.cpp:560-662) in Frame(n)
        // of the stored normal, whatever the side; the lobe choice (the
        // reference's sampler->next1D()) is dimension 7
        const float* st = S.refl + 3 * prim_bsdf<MESH>(S, q);
        const float wl[3] = {dot3(wi, s), dot3(wi, t), dot3(wi, n)};
        float bw[3], bpdf, crossed;
        roughdielectric_sample(wl, bp, st, rng_uniform(seed, gp, stream, 0), rng_uniform(seed, gp, stream, 1),
                               rng_uniform(seed, gp, stream, 7), w, bw, &bpdf, &crossed);
        Q.bw0[i] = bw[0]; Q.bw1[i] = bw[1]; Q.bw2[i] = bw[2];
        Q.bpdf[i] = bpdf;
        Q.beta[i] = crossed;
    } else if (DIEL && pure_delta) {
        // SmoothDielectric::sample / SmoothConductor::sample (bsdf_smooth.h)
        // with sample.x = dimension 0 (sample.y, dimension 1, is not read); a
        // void sample has weight 0
        const float* st = S.refl + 3 * prim_bsdf<MESH>(S, q);
        const float wl[3] = {dot3(wi, s), dot3(wi, t), dot3(wi, n)};
        float bw[3], bpdf, crossed;
        smooth_sample(wl, bp, st, rng_uniform(seed, gp, stream, 0), w, bw, &bpdf, &crossed);
        Q.bw0[i] = bw[0]; Q.bw1[i] = bw[1]; Q.bw2[i] = bw[2];
        Q.bpdf[i] = bpdf;
        Q.beta[i] = crossed;
        delta = 1;
    } else {
        cosine_hemisphere(rng_uniform(seed, gp, stream, 0), rng_uniform(seed, gp, stream, 1), w);
    }
    Q.bdelta[i] = delta;
    Q.b0[i] = s[0] * w[0] + t[0] * w[1] + n[0] * w[2];
    Q.b1[i] = s[1] * w[0] + t[1] * w[1] + n[1] * w[2];
    Q.b2[i] = s[2] * w[0] + t[2] * w[1] + n[2] * w[2];
    Q.u0[i] = rng_uniform(seed, gp, stream, 3);
    Q.u1[i] = rng_uniform(seed, gp, stream, 4);
    Q.u2[i] = rng_uniform(seed, gp, stream, 5);
    const float choice = rng_uniform(seed, gp, stream, 2);
    Q.ch[i] = choice;
    Q.mode[i] = (!guided || choice <= h) ? 1 : 0;
}

// the live guided queries, compacted: query j serves path idx[j].  With
// product sampling also the query's shading frame F = [s t n] (Frame(n) of
// the hit quad), its material (the quad's BSDF: its learned-BSDF table row;
// diffuse here, so getDMM succeeds for every live path, cosTheta(wi) > 0,
// bsdfs/diffuse.cpp:86-92; a rough conductor or a Phong BSDF: the query's own
// row of the extended table, its learned model conditioned here) and the
// BSDF/guide draw.
template <bool PHONG, bool DIEL, bool MESH, class... Nrm>
__global__ void __launch_bounds__(256)
li_compact_kernel(SceneDev S, PathsDev P, QueryDev Q, const int32_t* __restrict__ count, int product, Nrm... nrm) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= *count) return;
    const int i = Q.idx[j];
    Q.k_c0[j] = Q.c0[i]; Q.k_c1[j] = Q.c1[i]; Q.k_c2[j] = Q.c2[i];
    Q.k_u0[j] = Q.u0[i]; Q.k_u1[j] = Q.u1[i]; Q.k_u2[j] = Q.u2[i];
    Q.k_b0[j] = Q.b0[i]; Q.k_b1[j] = Q.b1[i]; Q.k_b2[j] = Q.b2[i];
    Q.k_mode[j] = Q.mode[i];
    Q.slot[i] = j;
    if (product) {
        float nbuf[3];
        const float* pn = path_ns<MESH>(S, i, P.quad[i], nbuf, nrm...);   // (NRM: F = [s t +-ns])
        const int qb = prim_bsdf<MESH>(S, P.quad[i]);
        float s[3], t[3];
        frame_of(pn, s, t);
        // a back hit on a two-sided BSDF: F = [s t -n] and the learned model
        // conditioned on the flipped local wi -- getDMM's negated column 2 of
        // `to` and mean.z (twosided.cpp:151-159) under [s t n]
        // (sdmm_proc.cpp:344-354) are the unflipped lobes under [s t -n]
        float qn[3] = {pn[0], pn[1], pn[2]};
        if (S.twosided) {
            const float wi[3] = {-P.dx[i], -P.dy[i], -P.dz[i]};
            if (twosided_back(S, qb, dot3(wi, qn)))
                for (int a = 0; a < 3; ++a) qn[a] = -qn[a];
        }
        for (int r = 0; r < 3; ++r) {
            Q.k_F[3 * r][j] = s[r];
            Q.k_F[3 * r + 1][j] = t[r];
            Q.k_F[3 * r + 2][j] = qn[r];
        }
        Q.k_mat[j] = qb;
        Q.k_ch[j] = Q.ch[i];
        const float* bp = S.bpar ? S.bpar + kBsdfParams * qb : nullptr;
        if (Q.lw && bp && bp[0] == (float)kBsdfConductor) {
            // getDMM (roughconductor.cpp:182-194: the material's SDMM4
            // conditioned on (theta_i, alpha), pruned to 2) + rotate_to_wo
            // (sdmm_proc.cpp:340-355): the query's own lobes, local frame, in
            // its row of the extended table; no model or no valid conditional:
            // no learned BSDF (the plain conditional, h 0.5)
            const float wi[3] = {-P.dx[i], -P.dy[i], -P.dz[i]};
            const float wl[3] = {dot3(wi, s), dot3(wi, t), dot3(wi, qn)};
            const int64_t row = (int64_t)Q.lrow0 + j;
            const float* lm = S.lmodel ? S.lmodel + (size_t)kLearnedStride * qb : nullptr;
            const int M = lm ? (int)lm[0] : 0;
            int kept = 0;
            if (M > 0) {
                const float theta = (float)acos((double)fminf(1.0f, wl[2]));
                kept = learned4_conditional(lm + 1, M, theta, bp[6], wl, kLearnedKeep, Q.lw + row * Q.lM,
                                            Q.lm + row * Q.lM * 3, Q.lc + row * Q.lM * 4);
            }
            for (int l = kept; l < Q.lM; ++l) Q.lw[row * Q.lM + l] = 0.0f;   // (skipped lobes)
            Q.k_mat[j] = kept > 0 ? (int32_t)row : -1;
        } else if (PHONG && Q.lw && bp && bp[0] == (float)kBsdfPhong) {
            // Phong::getDMM (phong.cpp:75-90: the material's SDMM5 conditioned
            // on (theta_i, max specular channel, log max(1, exponent)), pruned
            // to 2 with the diffuse component forced) + rotate_to_wo, into the
            // query's row as for the conductor
            const float wi[3] = {-P.dx[i], -P.dy[i], -P.dz[i]};
            const float wl[3] = {dot3(wi, s), dot3(wi, t), dot3(wi, qn)};
            const int64_t row = (int64_t)Q.lrow0 + j;
            const float* lm = S.lmodel_nd ? S.lmodel_nd + (size_t)kLearnedNdStride * qb : nullptr;
            const int M = lm ? (int)lm[1] : 0;
            int kept = 0;
            if (M > 0) {
                const float x[3] = {(float)acos((double)fminf(1.0f, wl[2])), fmaxf(bp[1], fmaxf(bp[2], bp[3])),
                                    (float)log((double)fmaxf(1.0f, bp[4]))};
                kept = learned_conditional<3>(lm + 2, M, x, wl, kLearnedKeep, kPhongDiffuseComponent,
                                              Q.lw + row * Q.lM, Q.lm + row * Q.lM * 3, Q.lc + row * Q.lM * 4);
            }
            for (int l = kept; l < Q.lM; ++l) Q.lw[row * Q.lM + l] = 0.0f;   // (skipped lobes)
            Q.k_mat[j] = kept > 0 ? (int32_t)row : -1;
        } else if (DIEL && Q.lw && bp && bp[0] == (float)kBsdfDielectric) {
            // RoughDielectric::getDMM (roughdielectric.cpp:198-211: the
            // material's SDMM5 conditioned on (theta_i, alpha, eta), pruned to
            // 2, no forced lobe) + rotate_to_wo, into the query's row as for
            // the conductor; a hit from inside (cosTheta(wi) <= 0, :199), no
            // model or no valid conditional: the plain conditional
            const float wi[3] = {-P.dx[i], -P.dy[i], -P.dz[i]};
            const float wl[3] = {dot3(wi, s), dot3(wi, t), dot3(wi, qn)};
            const int64_t row = (int64_t)Q.lrow0 + j;
            const float* lm = S.lmodel_nd ? S.lmodel_nd + (size_t)kLearnedNdStride * qb : nullptr;
            const int M = lm ? (int)lm[1] : 0;
            int kept = 0;
            if (M > 0 && wl[2] > 0.0f) {
                const float x[3] = {(float)acos((double)fminf(1.0f, wl[2])), bp[6], bp[4]};
                kept = learned_conditional<3>(lm + 2, M, x, wl, kLearnedKeep, -1, Q.lw + row * Q.lM,
                                              Q.lm + row * Q.lM * 3, Q.lc + row * Q.lM * 4);
            }
            for (int l = kept; l < Q.lM; ++l) Q.lw[row * Q.lM + l] = 0.0f;   // (skipped lobes)
            Q.k_mat[j] = kept > 0 ? (int32_t)row : -1;
        }
    }
}

// ---------------------------------------------------------------------------
// The rest of the bounce (:392-507, :759-871).
// product: the query's own heuristicConditionalWeight (0.3 with a usable
// product, 0.5 for the plain conditional, sdmm_proc.cpp:383-392) replaces h.
// The wavefront marks a query whose BSDF sample was chosen comp == -2 (valid
// conditional) -- the plain bounce's pdf_mode and the product bounce's
// choice <= h alike.
// ENV: the variant for a scene with an environment emitter, as the camera
// kernel's: a bounce ray that hits nothing brings evalEnvironment(wo) into
// `value` (rayIntersectAndLookForEmitter, :1047-1051) and the path ends.
// NRM: the variant for a mesh with vertex normals: the bounce runs on the
// hit's shading normal ns; strictNormals' second test is (wo . ng)
// cosTheta(bRec.wo) <= 0 (:777-780) with bRec.wo in its.shFrame -- twosided.cpp
// hands wo back with its z flipped again (:137) -- so (wo . ng)(wo . ns)
// whatever the side; without strictNormals neither test runs.  The new hit's
// ns / ng are worked out after the trace and left in the path's planes.
// TEX: the bounce weighs with the current hit's reflectance from the path's
// planes; the new hit's is looked up after the roulette and left there.
template <bool PHONG, bool DIEL, bool MESH, bool ENV, class... Nrm>
__global__ void __launch_bounds__(256)
li_shade_kernel(SceneDev S, PathsDev P, QueryDev Q, int64_t path0, int bounce, int rr_depth, float h,
                uint64_t seed, int product, Nrm... nrm) {
    constexpr bool NRM = pack_has<NormalsDev, Nrm...>, TEX = pack_has<TexDev, Nrm...>;
    static_assert(!NRM || MESH, "NRM: a MESH variant");
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.P) return;
    int depth = P.depth[i];
    if (depth < 0) return;
    LI_MESH_STACK(stack)
    const int pq = P.quad[i];
    float nbuf[3];
    const float* qn = path_ns<MESH>(S, i, pq, nbuf, nrm...);
    float n[3] = {qn[0], qn[1], qn[2]};
    // a two-sided BSDF met from behind: n is the effective normal -n from here
    // on (cosines, the saved vertex); the tangents stay Frame(qn)'s
    if (S.twosided) {
        const float wi[3] = {-P.dx[i], -P.dy[i], -P.dz[i]};
        if (twosided_back(S, prim_bsdf<MESH>(S, pq), dot3(wi, n)))
            for (int a = 0; a < 3; ++a) n[a] = -n[a];
    }
    // (TEX: the hit's own reflectance; a dielectric's row -- its
    // transmittance -- carries no texture and is read as ever)
    float rbuf[3];
    const float* rho_row = S.refl + 3 * prim_bsdf<MESH>(S, pq);
    const float* rho = path_rho(S, i, prim_bsdf<MESH>(S, pq), rbuf, nrm...);
    const int j = Q.slot[i];            // the path's guided query (-1: none, BSDF only)
    const int comp = j >= 0 ? Q.comp[j] : -1;
    const bool valid = comp != -1;      // validConditional (:368)
    if (product && valid) h = Q.hq[j];
    float wo[3], weight[3], mis_pdf;
    const float* bp = S.bpar ? S.bpar + kBsdfParams * prim_bsdf<MESH>(S, pq) : nullptr;
    bool cacheable = true;
    float crossed = 1.0f;               // bRec.eta (DIEL)
    bool inside = false;                // cosTheta(bRec.wi) < 0 (DIEL)
    if (bp && bp[0] == (float)kBsdfPlastic) {
        // smooth plastic (plastic.cpp): the loop head's sample (weight, pdf,
        // lobe) or the guide's direction under eval / pdf, the smooth part only
        const float wi[3] = {-P.dx[i], -P.dy[i], -P.dz[i]};
        const float Fi = fresnel_dielectric(dot3(wi, n), bp[4]);
        const float ps = plastic_prob_specular(Fi, bp[7]);
        const bool delta = Q.bdelta[i] != 0;
        const float bw[3] = {Q.bw0[i], Q.bw1[i], Q.bw2[i]};
        if (!valid || comp == -2) {
            wo[0] = Q.b0[i]; wo[1] = Q.b1[i]; wo[2] = Q.b2[i];
            cacheable = !delta;                 // :764
            if (!valid) {
                // BSDF only, h = 1 (:316-323, :392-405)
                mis_pdf = Q.bpdf[i];
                for (int ch = 0; ch < 3; ++ch) weight[ch] = bw[ch];
            } else if (delta) {
                // a delta lobe of the chosen BSDF sample: gmmPdf = 0, pdf *= h,
                // weight / h (:401-405)
                mis_pdf = Q.bpdf[i] * h;
                const float rh = 1.0f / h;
                for (int ch = 0; ch < 3; ++ch) weight[ch] = bw[ch] * rh;
            } else {
                // (bsdfWeight * bsdfPdf) / pdfSurface (:407, :531-534, :587-589)
                const float bsdf_pdf = Q.bpdf[i];
                mis_pdf = bsdf_pdf > 0.0f ? h * bsdf_pdf + (1.0f - h) * Q.pdf[j] : 0.0f;
                for (int ch = 0; ch < 3; ++ch) weight[ch] = mis_pdf == 0.0f ? 0.0f : (bw[ch] * bsdf_pdf) * (1.0f / mis_pdf);
            }
        } else {
            // the guide's direction: bsdf->eval (smooth lobe, ESolidAngle) / pdfSurface (:456-507)
            wo[0] = Q.d0[j]; wo[1] = Q.d1[j]; wo[2] = Q.d2[j];
            const float cos_o = dot3(wo, n);
            const bool zero = (wo[0] == 0.0f && wo[1] == 0.0f && wo[2] == 0.0f) || !__builtin_isfinite(cos_o);
            const bool up = !zero && cos_o > 0.0f;
            const float cpdf = kInvPi * cos_o;   // warp::squareToCosineHemispherePdf
            const float bsdf_pdf = up ? cpdf * (1.0f - ps) : 0.0f;
            mis_pdf = bsdf_pdf > 0.0f ? h * bsdf_pdf + (1.0f - h) * Q.pdf[j] : 0.0f;
            const float Fo = up ? fresnel_dielectric(cos_o, bp[4]) : 0.0f;
            const float rd = 1.0f / (1.0f - bp[6]);
            const float k = cpdf * bp[5] * (1.0f - Fi) * (1.0f - Fo);
            for (int ch = 0; ch < 3; ++ch) {
                const float f = up ? rho[ch] * rd * k : 0.0f;
                weight[ch] = mis_pdf == 0.0f ? 0.0f : f * (1.0f / mis_pdf);
            }
        }
    } else if (bp && (bp[0] == (float)kBsdfConductor || (PHONG && bp[0] == (float)kBsdfPhong))) {
        // rough conductor, Phong: the loop head's sample (weight, pdf) or the
        // guide's direction under eval / pdf (:392-407, :456-507)
        const float bw[3] = {Q.bw0[i], Q.bw1[i], Q.bw2[i]};
        if (!valid || comp == -2) {
            wo[0] = Q.b0[i]; wo[1] = Q.b1[i]; wo[2] = Q.b2[i];
            const float bsdf_pdf = Q.bpdf[i];
            if (!valid) {
                mis_pdf = bsdf_pdf;
                for (int ch = 0; ch < 3; ++ch) weight[ch] = bw[ch];
            } else {
                mis_pdf = bsdf_pdf > 0.0f ? h * bsdf_pdf + (1.0f - h) * Q.pdf[j] : 0.0f;
                for (int ch = 0; ch < 3; ++ch) weight[ch] = mis_pdf == 0.0f ? 0.0f : (bw[ch] * bsdf_pdf) * (1.0f / mis_pdf);
            }
        } else {
            wo[0] = Q.d0[j]; wo[1] = Q.d1[j]; wo[2] = Q.d2[j];
            float s[3], t[3];
            frame_of(qn, s, t);
            const float wi[3] = {-P.dx[i], -P.dy[i], -P.dz[i]};
            const float wil[3] = {dot3(wi, s), dot3(wi, t), dot3(wi, n)};
            const float wol[3] = {dot3(wo, s), dot3(wo, t), dot3(wo, n)};
            const bool zero = (wo[0] == 0.0f && wo[1] == 0.0f && wo[2] == 0.0f) || !__builtin_isfinite(wol[2]);
            float f[3] = {0.0f, 0.0f, 0.0f};
            const float bsdf_pdf = zero ? 0.0f
                                   : PHONG && bp[0] == (float)kBsdfPhong ? phong_eval_pdf(wil, wol, bp, rho, f)
                                                                : conductor_eval_pdf(wil, wol, bp, f);
            mis_pdf = bsdf_pdf > 0.0f ? h * bsdf_pdf + (1.0f - h) * Q.pdf[j] : 0.0f;
            for (int ch = 0; ch < 3; ++ch) weight[ch] = mis_pdf == 0.0f ? 0.0f : f[ch] * (1.0f / mis_pdf);
        }
    } else if (DIEL && bp && bp[0] == (float)kBsdfDielectric) {
        // rough dielectric: as the conductor, on the whole sphere -- the
        // guide's direction may lie below the surface, and the relative index
        // it crosses is what sample would have set for it (the reference's
        // bRec.eta is uninitialised there, records.inl:24-27)
        const float bw[3] = {Q.bw0[i], Q.bw1[i], Q.bw2[i]};
        const float wi[3] = {-P.dx[i], -P.dy[i], -P.dz[i]};
        inside = dot3(wi, n) < 0.0f;
        if (!valid || comp == -2) {
            wo[0] = Q.b0[i]; wo[1] = Q.b1[i]; wo[2] = Q.b2[i];
            crossed = Q.beta[i];
            const float bsdf_pdf = Q.bpdf[i];
            if (!valid) {
                mis_pdf = bsdf_pdf;
                for (int ch = 0; ch < 3; ++ch) weight[ch] = bw[ch];
            } else {
                mis_pdf = bsdf_pdf > 0.0f ? h * bsdf_pdf + (1.0f - h) * Q.pdf[j] : 0.0f;
                for (int ch = 0; ch < 3; ++ch) weight[ch] = mis_pdf == 0.0f ? 0.0f : (bw[ch] * bsdf_pdf) * (1.0f / mis_pdf);
            }
        } else {
            wo[0] = Q.d0[j]; wo[1] = Q.d1[j]; wo[2] = Q.d2[j];
            float s[3], t[3];
            frame_of(qn, s, t);
            const float wil[3] = {dot3(wi, s), dot3(wi, t), dot3(wi, n)};
            const float wol[3] = {dot3(wo, s), dot3(wo, t), dot3(wo, n)};
            const bool zero = (wo[0] == 0.0f && wo[1] == 0.0f && wo[2] == 0.0f) || !__builtin_isfinite(wol[2]);
            float f[3] = {0.0f, 0.0f, 0.0f};
            const float bsdf_pdf = zero ? 0.0f : roughdielectric_eval_pdf(wil, wol, bp, rho_row, f);
            crossed = roughdielectric_crossed_eta(wil, wol, bp);
            mis_pdf = bsdf_pdf > 0.0f ? h * bsdf_pdf + (1.0f - h) * Q.pdf[j] : 0.0f;
            for (int ch = 0; ch < 3; ++ch) weight[ch] = mis_pdf == 0.0f ? 0.0f : f[ch] * (1.0f / mis_pdf);
        }
    } else if (DIEL && bp && is_smooth_kind(bp[0])) {
        // smooth dielectric, smooth conductor: the whole BSDF is delta -- the
        // loop head's sample as it is (pdf = bsdfPdf, no guide query: slot -1;
        // :297-302), no saved vertex (:764)
        const float wi[3] = {-P.dx[i], -P.dy[i], -P.dz[i]};
        inside = dot3(wi, n) < 0.0f;
        wo[0] = Q.b0[i]; wo[1] = Q.b1[i]; wo[2] = Q.b2[i];
        crossed = Q.beta[i];
        mis_pdf = Q.bpdf[i];
        weight[0] = Q.bw0[i]; weight[1] = Q.bw1[i]; weight[2] = Q.bw2[i];
        cacheable = false;
    } else if (!valid) {
        // BSDF only, h = 1 (:316-323, :392-405): weight = rho, pdf = bsdfPdf
        wo[0] = Q.b0[i]; wo[1] = Q.b1[i]; wo[2] = Q.b2[i];
        const float cos_o = dot3(wo, n);
        mis_pdf = kInvPi * cos_o;
        for (int ch = 0; ch < 3; ++ch) weight[ch] = rho[ch];
    } else if (comp == -2) {
        // BSDF chosen: (bsdf weight * bsdfPdf) / (h bsdfPdf + (1 - h) gmmPdf) (:393-407, :587-589)
        wo[0] = Q.b0[i]; wo[1] = Q.b1[i]; wo[2] = Q.b2[i];
        const float bsdf_pdf = kInvPi * dot3(wo, n);
        mis_pdf = bsdf_pdf > 0.0f ? h * bsdf_pdf + (1.0f - h) * Q.pdf[j] : 0.0f;   // pdfSurface (:531-534)
        for (int ch = 0; ch < 3; ++ch) weight[ch] = mis_pdf == 0.0f ? 0.0f : (rho[ch] * bsdf_pdf) * (1.0f / mis_pdf);
    } else {
        // guide sample: bsdf->eval / pdf (:456-463, :504-507)
        wo[0] = Q.d0[j]; wo[1] = Q.d1[j]; wo[2] = Q.d2[j];
        const float cos_o = dot3(wo, n);
        const bool zero = (wo[0] == 0.0f && wo[1] == 0.0f && wo[2] == 0.0f) || !__builtin_isfinite(cos_o);
        const float bsdf_pdf = (!zero && cos_o > 0.0f) ? kInvPi * cos_o : 0.0f;
        mis_pdf = bsdf_pdf > 0.0f ? h * bsdf_pdf + (1.0f - h) * Q.pdf[j] : 0.0f;   // pdfSurface (:531-534)
        for (int ch = 0; ch < 3; ++ch) weight[ch] = mis_pdf == 0.0f ? 0.0f : (rho[ch] * (kInvPi * cos_o)) * (1.0f / mis_pdf);
    }
    const float cos_o = dot3(wo, n);
    // zero weight, or strict normals (wo . n_geo * cos(wo) <= 0, :777-780): the path ends
    bool leak = !(cos_o * cos_o > 0.0f);
    if constexpr (NRM) {
        const NormalsDev N = nrm_arg(nrm...);
        const float ng[3] = {N.ngx[i], N.ngy[i], N.ngz[i]};
        leak = N.strict && !(dot3(wo, ng) * dot3(wo, qn) > 0.0f);
    }
    if ((weight[0] == 0.0f && weight[1] == 0.0f && weight[2] == 0.0f) || leak ||
        !__builtin_isfinite(weight[0] + weight[1] + weight[2])) {
        P.depth[i] = -1;
        return;
    }
    float thr[3] = {P.tr[i] * weight[0], P.tg[i] * weight[1], P.tb[i] * weight[2]};
    // trace and look for an emitter (rayIntersectAndLookForEmitter)
    const float o[3] = {P.px[i], P.py[i], P.pz[i]};
    float t;
    const int q = intersect<MESH>(S, o, wo, kEpsilon, INFINITY, t, stack);
    float value[3] = {0.0f, 0.0f, 0.0f};
    float hns[3], hng[3];               // the new hit's normals (NRM)
    float huv[2];                       // ... and its uv (NRM and TEX: from the same triangle test)
    if (q >= 0) {
        const int he = prim_emitter<MESH>(S, q);
        const float* hn;
        if constexpr (NRM) {
            if constexpr (!TEX) hit_normals(S, nrm_arg(nrm...).shade, q, o, wo, hns, hng);
            else hit_normals_uv(S, nrm_arg(nrm...).shade, tex_arg(nrm...).mesh_uv, q, o, wo, hns, hng, huv);
            hn = hns;
        } else {
            hn = prim_n<MESH>(S, q);
        }
        if (he >= 0 && -dot3(wo, hn) > 0.0f)
            for (int ch = 0; ch < 3; ++ch) value[ch] = S.rad[3 * he + ch];
    }
    if constexpr (ENV)
        if (q < 0) env_eval<true>(S.env, wo, value);
    int nv = P.nv[i];
    if (value[0] != 0.0f || value[1] != 0.0f || value[2] != 0.0f) {
        const float rad[3] = {thr[0] * value[0], thr[1] * value[1], thr[2] * value[2]};
        P.lr[i] += rad[0]; P.lg[i] += rad[1]; P.lb[i] += rad[2];
        record_radiance(P, i, nv, rad);
    }
    P.nray[i] += 1;
    // the saved vertex (cacheable: not a delta lobe, :764, :821-845)
    if (cacheable && nv < P.V) {
        // (the condition is read here, not at the top: it is needed nowhere
        // else, and its three registers stay free over the bounce and the trace)
        const float c[3] = {Q.c0[i], Q.c1[i], Q.c2[i]};
        const float clamped = fmaxf(mis_pdf, 0.1f);
        const float inv_pdf = 1.0f / clamped;
        for (int ch = 0; ch < 3; ++ch) {
            vrec(P, ch, nv, i) = value[ch] * inv_pdf;
            vrec(P, 3 + ch, nv, i) = thr[ch];
        }
        vrec(P, 6, nv, i) = clamped;
        for (int a = 0; a < 3; ++a) {
            vrec(P, 7 + a, nv, i) = c[a];
            vrec(P, 10 + a, nv, i) = wo[a];
            // (inside a dielectric the vertex carries the inward normal,
            // :765-767; behind a two-sided BSDF n already is the flipped one)
            vrec(P, 13 + a, nv, i) = DIEL && inside ? -n[a] : n[a];
        }
        P.nv[i] = nv + 1;
    }
    // Russian roulette (:858-868)
    bool live = q >= 0;
    float eta = 1.0f;                   // the path's relative index (:788)
    if (DIEL) {
        eta = P.eta[i] * crossed;
        P.eta[i] = eta;
    }
    if (depth >= rr_depth && live) {
        const float tmax = fmaxf(thr[0], fmaxf(thr[1], thr[2]));
        const float qq = fminf(DIEL ? tmax * eta * eta : tmax, 0.95f);   // (:864)
        if (rng_uniform(seed, (uint64_t)(path0 + i), 1u + (uint32_t)bounce, 6) >= qq) live = false;
        else for (int ch = 0; ch < 3; ++ch) thr[ch] /= qq;
    }
    P.tr[i] = thr[0]; P.tg[i] = thr[1]; P.tb[i] = thr[2];
    P.dx[i] = wo[0]; P.dy[i] = wo[1]; P.dz[i] = wo[2];
    if (live) {
        P.px[i] = o[0] + t * wo[0]; P.py[i] = o[1] + t * wo[1]; P.pz[i] = o[2] + t * wo[2];
        P.quad[i] = q;
        if constexpr (NRM) store_normals(nrm_arg(nrm...), i, hns, hng);
        // (TEX: the lookup here, for the paths that go on -- nothing of it is
        // live over the bounce and the trace)
        if constexpr (TEX) {
            if constexpr (!NRM) hit_uv(S.quads, S.n_quads, tex_arg(nrm...).mesh_uv, q, o, wo, huv);
            store_reflectance(S, tex_arg(nrm...), i, prim_bsdf<MESH>(S, q), huv);
        }
    }
    P.depth[i] = live ? depth + 1 : -1;
}

// pixel mean over its spp samples, in sample order; image planes [3][W*H];
// image_sqr (nullable): the mean of the squared samples (the reference's
// m_blockSqr, sdmm_wr.cpp:144-145)
__global__ void __launch_bounds__(256)
li_film_kernel(PathsDev P, int64_t pix0, int64_t npix, int spp, int64_t plane, float* __restrict__ image,
               float* __restrict__ image_sqr) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= npix) return;
    float acc[3] = {0.0f, 0.0f, 0.0f}, sq[3] = {0.0f, 0.0f, 0.0f};
    for (int s = 0; s < spp; ++s) {
        const int64_t i = j * spp + s;
        const float l[3] = {P.lr[i], P.lg[i], P.lb[i]};
        for (int ch = 0; ch < 3; ++ch) {
            acc[ch] += l[ch];
            sq[ch] += l[ch] * l[ch];
        }
    }
    const float inv = 1.0f / (float)spp;
    for (int ch = 0; ch < 3; ++ch) image[ch * plane + pix0 + j] = acc[ch] * inv;
    if (image_sqr)
        for (int ch = 0; ch < 3; ++ch) image_sqr[ch * plane + pix0 + j] = sq[ch] * inv;
}

// ---------------------------------------------------------------------------
// Training-data producer (:876-965).  Per path, vertices d = nv-1 .. firstSaved:
// find its leaf (with the leaf's box), push (point, normal, average weight)
// there with a stats entry when the weight is finite (jmm isValidSample); then
// nJitters = (d == nv-1) + (average > 1000) pushes to the leaf at position +
// (u - 1/2) * leaf diagonal, a draw that lands outside the tree or in the same
// leaf (equal box min) retried while fewer than 8 draws failed.  Pass 0 counts
// a path's records, pass 1 writes (leaf, code) at its offset; code =
// ((path * V + d) << 1) | stats.  Records keep (path, push) order.
// a record staged in path order (48 B, one or two cache lines) for the
// leaf-order gather: point + wo, normal, average weight, code
struct alignas(16) ProducedRec {
    float x[6];
    float n[3];
    float w;
    int64_t code;
};
static_assert(sizeof(ProducedRec) == 48, "ProducedRec layout");

template <bool WRITE>
__device__ __forceinline__ int produce_path(const STNodeDev* __restrict__ nodes, const PathsDev& P, int64_t p,
                                            int64_t path0, int saved, uint64_t seed, uint32_t* keys,
                                            int64_t* codes, ProducedRec* recs, int64_t off, int* lost) {
    const int nv = P.nv[p];
    const int first = nv - saved > 0 ? nv - saved : 0;
    int cnt = 0;
    for (int d = nv - 1; d >= first; --d) {
        const float pos[3] = {vrec(P, 7, d, p), vrec(P, 8, d, p), vrec(P, 9, d, p)};
        const int leaf = stree_find_point(nodes, pos[0], pos[1], pos[2]);
        if (leaf < 0) {   // the reference throws (:924-930)
            if (WRITE) atomicAdd(lost, 1);
            continue;
        }
        const STNodeDev box = nodes[leaf];
        const float avg = (vrec(P, 0, d, p) + vrec(P, 1, d, p) + vrec(P, 2, d, p)) * (1.0f / 3.0f);
        const bool ok = __builtin_isfinite(avg);
        const int64_t code = ((int64_t)p * P.V + d) << 1;
        ProducedRec r{};
        if (WRITE && ok) {
            for (int a = 0; a < 3; ++a) {
                r.x[a] = pos[a];
                r.x[3 + a] = vrec(P, 10 + a, d, p);
                r.n[a] = vrec(P, 13 + a, d, p);
            }
            r.w = avg;
        }
        auto put = [&](uint32_t key, int64_t c) {
            const int64_t at = off + cnt;
            keys[at] = key;
            codes[at] = at;   // the sort's payload: the staged record's slot
            r.code = c;
            recs[at] = r;
        };
        if (ok) {
            if (WRITE) put((uint32_t)leaf, code | 1);
            ++cnt;
        }
        int jitters = (d >= nv - 1 ? 1 : 0) + (avg > 1000.0f ? 1 : 0);
        int attempts = 0, draw = 0;
        const float diag[3] = {box.mx[0] - box.mn[0], box.mx[1] - box.mn[1], box.mx[2] - box.mn[2]};
        for (int j = 0; j < jitters; ++j) {
            const uint64_t gp = (uint64_t)(path0 + p);
            float jp[3];
            for (int a = 0; a < 3; ++a)
                jp[a] = pos[a] + (rng_uniform(seed, gp, kJitterStream + (uint32_t)d, 3 * draw + a) - 0.5f) * diag[a];
            ++draw;
            const int nb = stree_find_point(nodes, jp[0], jp[1], jp[2]);
            bool same = nb < 0;
            if (!same) {
                const STNodeDev b = nodes[nb];
                same = b.mn[0] == box.mn[0] && b.mn[1] == box.mn[1] && b.mn[2] == box.mn[2];
            }
            if (same) {
                ++attempts;
                if (attempts < 8) --j;
                continue;
            }
            if (ok) {
                if (WRITE) put((uint32_t)nb, code);
                ++cnt;
            }
        }
    }
    return cnt;
}

__global__ void __launch_bounds__(256)
produce_count_kernel(const STNodeDev* __restrict__ nodes, PathsDev P, int64_t path0, int saved, uint64_t seed,
                     int64_t* __restrict__ count) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P.P) return;
    count[p] = produce_path<false>(nodes, P, p, path0, saved, seed, nullptr, nullptr, nullptr, 0, nullptr);
}

__global__ void __launch_bounds__(256)
produce_write_kernel(const STNodeDev* __restrict__ nodes, PathsDev P, int64_t path0, int saved, uint64_t seed,
                     const int64_t* __restrict__ offset, uint32_t* __restrict__ keys, int64_t* __restrict__ codes,
                     ProducedRec* __restrict__ recs, int* __restrict__ lost) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P.P) return;
    (void)produce_path<true>(nodes, P, p, path0, saved, seed, keys, codes, recs, offset[p], lost);
}

// leaf-contiguous records -> training planes (slot: the staged record of
// sorted position j)
__global__ void __launch_bounds__(256)
produce_gather_kernel(const ProducedRec* __restrict__ recs, const int64_t* __restrict__ slot, int64_t n, float* x0,
                      float* x1, float* x2, float* x3, float* x4, float* x5, float* n0, float* n1, float* n2,
                      float* w, uint8_t* stats, const uint32_t* __restrict__ keys, int32_t* node, int64_t* source) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const ProducedRec r = recs[slot[j]];
    x0[j] = r.x[0]; x1[j] = r.x[1]; x2[j] = r.x[2];
    x3[j] = r.x[3]; x4[j] = r.x[4]; x5[j] = r.x[5];
    if (n0) { n0[j] = r.n[0]; n1[j] = r.n[1]; n2[j] = r.n[2]; }
    w[j] = r.w;
    if (stats) stats[j] = (uint8_t)(r.code & 1);
    if (node) node[j] = (int32_t)keys[j];
    if (source) source[j] = r.code >> 1;   // p * V + d
}

// seg[v] = first sorted position with key >= v, v = 0..num_nodes
__global__ void produce_seg_kernel(const uint32_t* __restrict__ keys, int64_t n, int num_nodes,
                                   int64_t* __restrict__ seg) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v > num_nodes) return;
    int64_t lo = 0, count = n;
    while (count > 0) {
        const int64_t step = count / 2, it = lo + step;
        if (keys[it] < (uint32_t)v) { lo = it + 1; count -= step + 1; }
        else count = step;
    }
    seg[v] = lo;
}

// ---------------------------------------------------------------------------
// host launchers
static inline dim3 grid_for(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }
// f(std::true_type{}) or f(std::false_type{}): a run-time flag as a template argument
template <class F>
static void with_flag(bool flag, F f) {
    if (flag) f(std::true_type{});
    else f(std::false_type{});
}
// The Li kernel variant of a scene, stated once: launch(phong, diel, mesh, env,
// nrm...) gets, as std::bool_constant values, PHONG = some BSDF is Phong, DIEL =
// some is a dielectric or delta only, MESH = the scene has triangles, ENV = it
// has an environment emitter (ENV_KERNEL: the camera and shade kernels; false
// for the others), and the pack nrm: N with vertex normals (N.shade set: the
// NRM variants, always MESH), then T with textured BSDFs (T.bsdf_tex set: the
// TEX variants; TEX_KERNEL: the camera, query and shade kernels -- compact
// reads nothing of T and has no such variant), nothing otherwise.  (The nesting -- NRM, ENV, MESH, DIEL,
// PHONG, TEX, true first -- is the order the variants are instantiated in, and
// so the order of the kernels in the code object.)
template <bool ENV_KERNEL, bool TEX_KERNEL, class F>
static void li_variant(const SceneDev& S, const NormalsDev& N, const TexDev& T, F launch) {
    const auto by_bsdfs = [&](auto env, auto mesh, auto... nrm) {
        with_flag(S.has_dielectric, [&](auto diel) {
            with_flag(S.has_phong, [&](auto phong) {
                if constexpr (TEX_KERNEL) {
                    if (T.bsdf_tex) return launch(phong, diel, mesh, env, nrm..., T);
                }
                launch(phong, diel, mesh, env, nrm...);
            });
        });
    };
    const auto by_env = [&](auto next) {
        if constexpr (ENV_KERNEL) with_flag(S.env.kind != kEnvNone, next);
        else next(std::false_type{});
    };
    if (N.shade) by_env([&](auto env) { by_bsdfs(env, std::true_type{}, N); });
    else by_env([&](auto env) { with_flag(S.has_mesh, [&](auto mesh) { by_bsdfs(env, mesh); }); });
}

hipError_t launch_li_camera(const SceneDev& S, const PathsDev& P, const NormalsDev& N, const TexDev& T, int64_t path0,
                            int spp, uint64_t seed, hipStream_t st) {
    li_variant<true, true>(S, N, T, [&](auto, auto, auto mesh, auto env, auto... nrm) {
        hipLaunchKernelGGL((li_camera_kernel<mesh.value, env.value, decltype(nrm)...>), grid_for(P.P), dim3(256), 0, st,
                           S, P, path0, spp, seed, nrm...);
    });
    return hipGetLastError();
}
hipError_t launch_li_query(const SceneDev& S, const PathsDev& P, const QueryDev& Q, const NormalsDev& N,
                           const TexDev& T, int64_t path0, int bounce, int max_depth, int guided, float h,
                           uint64_t seed, hipStream_t st) {
    li_variant<false, true>(S, N, T, [&](auto phong, auto diel, auto mesh, auto, auto... nrm) {
        hipLaunchKernelGGL((li_query_kernel<phong.value, diel.value, mesh.value, decltype(nrm)...>), grid_for(P.P),
                           dim3(256), 0, st, S, P, Q, path0, bounce, max_depth, guided, h, seed, nrm...);
    });
    return hipGetLastError();
}
size_t li_select_temp_bytes(int64_t n) {
    size_t b = 0;
    (void)hipcub::DeviceSelect::Flagged(nullptr, b, hipcub::CountingInputIterator<int32_t>(0), (const uint8_t*)nullptr,
                                        (int32_t*)nullptr, (int32_t*)nullptr, (int)n);
    return b;
}
// live guided queries -> compact planes; *count_dev = their number
hipError_t launch_li_compact(const SceneDev& S, const PathsDev& P, const QueryDev& Q, const NormalsDev& N, int64_t n,
                             int32_t* count_dev, void* temp, size_t temp_bytes, int product, hipStream_t st) {
    hipError_t e = hipcub::DeviceSelect::Flagged(temp, temp_bytes, hipcub::CountingInputIterator<int32_t>(0), Q.live,
                                                 Q.idx, count_dev, (int)n, st);
    if (e != hipSuccess) return e;
    li_variant<false, false>(S, N, TexDev{}, [&](auto phong, auto diel, auto mesh, auto, auto... nrm) {
        hipLaunchKernelGGL((li_compact_kernel<phong.value, diel.value, mesh.value, decltype(nrm)...>), grid_for(n),
                           dim3(256), 0, st, S, P, Q, (const int32_t*)count_dev, product, nrm...);
    });
    return hipGetLastError();
}

hipError_t launch_li_shade(const SceneDev& S, const PathsDev& P, const QueryDev& Q, const NormalsDev& N,
                           const TexDev& T, int64_t path0, int bounce, int rr_depth, float h, uint64_t seed,
                           int product, hipStream_t st) {
    li_variant<true, true>(S, N, T, [&](auto phong, auto diel, auto mesh, auto env, auto... nrm) {
        hipLaunchKernelGGL((li_shade_kernel<phong.value, diel.value, mesh.value, env.value, decltype(nrm)...>),
                           grid_for(P.P), dim3(256), 0, st, S, P, Q, path0, bounce, rr_depth, h, seed, product, nrm...);
    });
    return hipGetLastError();
}

// sdmm_env_eval: evalEnvironment of nq directions on device planes
__global__ void __launch_bounds__(256)
env_eval_kernel(EnvDev E, int64_t nq, const float* __restrict__ d0, const float* __restrict__ d1,
                const float* __restrict__ d2, float* __restrict__ r, float* __restrict__ g, float* __restrict__ b) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const float d[3] = {d0[i], d1[i], d2[i]};
    float rgb[3];
    env_eval<true>(E, d, rgb);
    r[i] = rgb[0]; g[i] = rgb[1]; b[i] = rgb[2];
}
hipError_t launch_env_eval(const SceneDev& S, int64_t nq, const float* const d[3], float* const rgb[3],
                           hipStream_t st) {
    if (nq <= 0) return hipSuccess;
    hipLaunchKernelGGL(env_eval_kernel, grid_for(nq), dim3(256), 0, st, S.env, nq, d[0], d[1], d[2], rgb[0], rgb[1],
                       rgb[2]);
    return hipGetLastError();
}
// getDMM + rotate_to_wo for a batch of local incident directions against one
// learned model (sdmm_learned4_conditional_device): query q's lobes at
// w[q * keep ..], mean[(q * keep + j) * 3 ..], cov[(q * keep + j) * 4 ..],
// its lobe count n[q] (0: no valid conditional, or cos theta_i <= 0)
struct Learned4Rec {
    float r[kLearnedMaxComp * kLearnedRec];
};
__global__ void __launch_bounds__(256)
learned4_kernel(Learned4Rec model, int M, float alpha, int64_t nq, const float* __restrict__ w0,
                const float* __restrict__ w1, const float* __restrict__ w2, int keep, float* __restrict__ w,
                float* __restrict__ mean, float* __restrict__ cov, int32_t* __restrict__ n) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    const float wl[3] = {w0[q], w1[q], w2[q]};
    int kept = 0;
    if (wl[2] > 0.0f) {
        const float theta = (float)acos((double)fminf(1.0f, wl[2]));
        float lw[kLearnedMaxComp], lm[3 * kLearnedMaxComp], lc[4 * kLearnedMaxComp];
        kept = learned4_conditional(model.r, M, theta, alpha, wl, keep, lw, lm, lc);
        for (int j = 0; j < kept; ++j) {
            w[q * keep + j] = lw[j];
            for (int i = 0; i < 3; ++i) mean[(q * keep + j) * 3 + i] = lm[3 * j + i];
            for (int i = 0; i < 4; ++i) cov[(q * keep + j) * 4 + i] = lc[4 * j + i];
        }
    }
    for (int j = kept; j < keep; ++j) w[q * keep + j] = 0.0f;
    n[q] = kept;
}
hipError_t launch_learned4(const float* rec, int M, float alpha, int64_t nq, const float* const wl[3], int keep,
                           float* w, float* mean, float* cov, int32_t* n, hipStream_t st) {
    if (M < 0 || M > kLearnedMaxComp || keep < 1 || keep > kLearnedMaxComp) return hipErrorInvalidValue;
    if (nq <= 0) return hipSuccess;
    Learned4Rec m{};
    for (int i = 0; i < M * kLearnedRec; ++i) m.r[i] = rec[i];
    hipLaunchKernelGGL(learned4_kernel, grid_for(nq), dim3(256), 0, st, m, M, alpha, nq, wl[0], wl[1], wl[2], keep, w,
                       mean, cov, n);
    return hipGetLastError();
}

// The same over a condition of dimension C (sdmm_learned_conditional_device):
// query q's condition is (theta_i, rest[0][q] .. rest[C-2][q]), a null plane
// broadcasting scal[i]; rows lobes a query (keep, or kLearnedMaxComp when
// keep is 0: unpruned)
struct LearnedNdRec {
    float r[kLearnedMaxComp * learned_rec(kLearnedMaxCond)];
};
struct LearnedNdCond {
    const float* rest[kLearnedMaxCond - 1];
    float scal[kLearnedMaxCond - 1];
};
template <int C>
__global__ void __launch_bounds__(256)
learned_nd_kernel(LearnedNdRec model, int M, LearnedNdCond cond, int64_t nq, const float* __restrict__ w0,
                  const float* __restrict__ w1, const float* __restrict__ w2, int keep, int force, int rows,
                  float* __restrict__ w, float* __restrict__ mean, float* __restrict__ cov, int32_t* __restrict__ n) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    const float wl[3] = {w0[q], w1[q], w2[q]};
    int kept = 0;
    if (wl[2] > 0.0f) {
        float x[C];
        x[0] = (float)acos((double)fminf(1.0f, wl[2]));
        for (int i = 0; i < C - 1; ++i) x[1 + i] = cond.rest[i] ? cond.rest[i][q] : cond.scal[i];
        float lw[kLearnedMaxComp], lm[3 * kLearnedMaxComp], lc[4 * kLearnedMaxComp];
        kept = learned_conditional<C>(model.r, M, x, wl, keep, force, lw, lm, lc);
        for (int j = 0; j < kept; ++j) {
            w[q * rows + j] = lw[j];
            for (int i = 0; i < 3; ++i) mean[(q * rows + j) * 3 + i] = lm[3 * j + i];
            for (int i = 0; i < 4; ++i) cov[(q * rows + j) * 4 + i] = lc[4 * j + i];
        }
    }
    for (int j = kept; j < rows; ++j) w[q * rows + j] = 0.0f;
    n[q] = kept;
}
hipError_t launch_learned_nd(int C, const float* rec, int M, const float* const* rest, const float* scal, int64_t nq,
                             const float* const wl[3], int keep, int force, float* w, float* mean, float* cov,
                             int32_t* n, hipStream_t st) {
    if ((C != 2 && C != 3) || M < 0 || M > kLearnedMaxComp || keep < 0 || keep > kLearnedMaxComp || force < -1 ||
        (force >= 0 && force >= M))
        return hipErrorInvalidValue;
    if (nq <= 0) return hipSuccess;
    LearnedNdRec m{};
    for (int i = 0; i < M * learned_rec(C); ++i) m.r[i] = rec[i];
    LearnedNdCond cond{};
    for (int i = 0; i < C - 1; ++i) {
        cond.rest[i] = rest ? rest[i] : nullptr;
        cond.scal[i] = scal ? scal[i] : 0.0f;
    }
    const int rows = keep == 0 ? kLearnedMaxComp : keep;
    if (C == 2)
        hipLaunchKernelGGL(learned_nd_kernel<2>, grid_for(nq), dim3(256), 0, st, m, M, cond, nq, wl[0], wl[1], wl[2],
                           keep, force, rows, w, mean, cov, n);
    else
        hipLaunchKernelGGL(learned_nd_kernel<3>, grid_for(nq), dim3(256), 0, st, m, M, cond, nq, wl[0], wl[1], wl[2],
                           keep, force, rows, w, mean, cov, n);
    return hipGetLastError();
}

// The rough dielectric BSDF over a batch of local incident directions
// (sdmm_bsdf_roughdielectric_device): sample mode draws wo from (u0, u1, u2),
// eval mode (u0 null) evaluates the given wo; each query as the host call
struct DielectricArgs {
    float bp[kBsdfParams];
    float st[3];
};
__global__ void __launch_bounds__(256)
roughdielectric_kernel(DielectricArgs A, int64_t nq, const float* __restrict__ wi0, const float* __restrict__ wi1,
                       const float* __restrict__ wi2, const float* __restrict__ u0, const float* __restrict__ u1,
                       const float* __restrict__ u2, float* wo0, float* wo1, float* wo2, float* __restrict__ v0,
                       float* __restrict__ v1, float* __restrict__ v2, float* __restrict__ pdf,
                       float* __restrict__ eta_out) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    const float wi[3] = {wi0[q], wi1[q], wi2[q]};
    float wo[3], f[3], p, e;
    if (u0) {
        roughdielectric_sample(wi, A.bp, A.st, u0[q], u1[q], u2[q], wo, f, &p, &e);
        wo0[q] = wo[0]; wo1[q] = wo[1]; wo2[q] = wo[2];
    } else {
        wo[0] = wo0[q]; wo[1] = wo1[q]; wo[2] = wo2[q];
        p = roughdielectric_eval_pdf(wi, wo, A.bp, A.st, f);
        e = roughdielectric_crossed_eta(wi, wo, A.bp);
    }
    v0[q] = f[0]; v1[q] = f[1]; v2[q] = f[2];
    pdf[q] = p;
    eta_out[q] = e;
}
hipError_t launch_roughdielectric(const float* bp, const float st[3], int64_t nq, const float* const wi[3],
                                  const float* const* u, float* const wo[3], float* const value[3], float* pdf,
                                  float* eta_out, hipStream_t st_) {
    if (nq <= 0) return hipSuccess;
    DielectricArgs A{};
    for (int i = 0; i < kBsdfParams; ++i) A.bp[i] = bp[i];
    for (int i = 0; i < 3; ++i) A.st[i] = st[i];
    hipLaunchKernelGGL(roughdielectric_kernel, grid_for(nq), dim3(256), 0, st_, A, nq, wi[0], wi[1], wi[2],
                       u ? u[0] : nullptr, u ? u[1] : nullptr, u ? u[2] : nullptr, wo[0], wo[1], wo[2], value[0],
                       value[1], value[2], pdf, eta_out);
    return hipGetLastError();
}

// The delta-only BSDFs (bsdf_smooth.h) over a batch of local incident
// directions (sdmm_bsdf_smooth_device): sample mode draws wo from u0 (u1 is
// not read), eval mode (u0 null) evaluates the given wo; each query as the
// host call
__global__ void __launch_bounds__(256)
smooth_kernel(DielectricArgs A, int64_t nq, const float* __restrict__ wi0, const float* __restrict__ wi1,
              const float* __restrict__ wi2, const float* __restrict__ u0, float* wo0, float* wo1, float* wo2,
              float* __restrict__ v0, float* __restrict__ v1, float* __restrict__ v2, float* __restrict__ pdf,
              float* __restrict__ eta_out) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    const float wi[3] = {wi0[q], wi1[q], wi2[q]};
    float wo[3], f[3], p, e;
    if (u0) {
        smooth_sample(wi, A.bp, A.st, u0[q], wo, f, &p, &e);
        wo0[q] = wo[0]; wo1[q] = wo[1]; wo2[q] = wo[2];
    } else {
        wo[0] = wo0[q]; wo[1] = wo1[q]; wo[2] = wo2[q];
        p = smooth_eval_pdf(wi, wo, A.bp, A.st, f, &e);
    }
    v0[q] = f[0]; v1[q] = f[1]; v2[q] = f[2];
    pdf[q] = p;
    eta_out[q] = e;
}
hipError_t launch_smooth(const float* bp, const float st[3], int64_t nq, const float* const wi[3],
                         const float* const* u, float* const wo[3], float* const value[3], float* pdf,
                         float* eta_out, hipStream_t st_) {
    if (nq <= 0) return hipSuccess;
    DielectricArgs A{};
    for (int i = 0; i < kBsdfParams; ++i) A.bp[i] = bp[i];
    for (int i = 0; i < 3; ++i) A.st[i] = st ? st[i] : 0.0f;
    hipLaunchKernelGGL(smooth_kernel, grid_for(nq), dim3(256), 0, st_, A, nq, wi[0], wi[1], wi[2],
                       u ? u[0] : nullptr, wo[0], wo[1], wo[2], value[0], value[1], value[2], pdf, eta_out);
    return hipGetLastError();
}

// sdmm_scene_intersect: the closest hit of nq rays on device planes, quads by
// their loop, then the triangles through the BVH (BRUTE: the loop over all)
template <bool BRUTE>
__global__ void __launch_bounds__(256)
scene_intersect_kernel(SceneDev S, int64_t nq, const float* __restrict__ o0, const float* __restrict__ o1,
                       const float* __restrict__ o2, const float* __restrict__ d0, const float* __restrict__ d1,
                       const float* __restrict__ d2, float mint, float maxt, int32_t* __restrict__ prim,
                       float* __restrict__ t_out) {
    __shared__ int bvh_lds[BRUTE ? 1 : kBvhStack * 256];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const float o[3] = {o0[i], o1[i], o2[i]}, d[3] = {d0[i], d1[i], d2[i]};
    float t;
    int best = quads_closest(S.quads, S.n_quads, o, d, mint, maxt, t);
    if (S.n_tris > 0) {
        if (BRUTE) {
            mesh_brute(S.tris, S.n_tris, S.n_quads, o, d, mint, maxt, best, t);
        } else {
            LdsStack st{bvh_lds + threadIdx.x};
            bvh_closest(S.nodes, S.tris, S.n_quads, o, d, mint, maxt, best, t, st);
        }
    }
    prim[i] = best;
    t_out[i] = t;
}
hipError_t launch_scene_intersect(const SceneDev& S, int64_t nq, const float* const o[3], const float* const d[3],
                                  float mint, float maxt, int mode, int32_t* prim, float* t, hipStream_t st) {
    if (nq <= 0) return hipSuccess;
    if (mode == 0)
        hipLaunchKernelGGL(scene_intersect_kernel<false>, grid_for(nq), dim3(256), 0, st, S, nq, o[0], o[1], o[2],
                           d[0], d[1], d[2], mint, maxt, prim, t);
    else
        hipLaunchKernelGGL(scene_intersect_kernel<true>, grid_for(nq), dim3(256), 0, st, S, nq, o[0], o[1], o[2],
                           d[0], d[1], d[2], mint, maxt, prim, t);
    return hipGetLastError();
}

// sdmm_scene_shading: sdmm_scene_intersect's search, then the hit's shading
// and geometric normal as the Li kernels compute them (hit_normals); zeros on
// a miss
template <bool BRUTE>
__global__ void __launch_bounds__(256)
scene_shading_kernel(SceneDev S, const MeshShade* __restrict__ shade, int64_t nq, const float* __restrict__ o0, const float* __restrict__ o1,
                     const float* __restrict__ o2, const float* __restrict__ d0, const float* __restrict__ d1,
                     const float* __restrict__ d2, float mint, float maxt, int32_t* __restrict__ prim,
                     float* __restrict__ t_out, float* __restrict__ ns0, float* __restrict__ ns1,
                     float* __restrict__ ns2, float* __restrict__ ng0, float* __restrict__ ng1,
                     float* __restrict__ ng2) {
    __shared__ int bvh_lds[BRUTE ? 1 : kBvhStack * 256];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const float o[3] = {o0[i], o1[i], o2[i]}, d[3] = {d0[i], d1[i], d2[i]};
    float t;
    int best = quads_closest(S.quads, S.n_quads, o, d, mint, maxt, t);
    if (S.n_tris > 0) {
        if (BRUTE) {
            mesh_brute(S.tris, S.n_tris, S.n_quads, o, d, mint, maxt, best, t);
        } else {
            LdsStack st{bvh_lds + threadIdx.x};
            bvh_closest(S.nodes, S.tris, S.n_quads, o, d, mint, maxt, best, t, st);
        }
    }
    float ns[3] = {0.0f, 0.0f, 0.0f}, ng[3] = {0.0f, 0.0f, 0.0f};
    if (best >= 0) hit_normals(S, shade, best, o, d, ns, ng);
    prim[i] = best;
    t_out[i] = t;
    ns0[i] = ns[0]; ns1[i] = ns[1]; ns2[i] = ns[2];
    ng0[i] = ng[0]; ng1[i] = ng[1]; ng2[i] = ng[2];
}
hipError_t launch_scene_shading(const SceneDev& S, const MeshShade* shade, int64_t nq, const float* const o[3],
                                const float* const d[3], float mint, float maxt, int mode, int32_t* prim, float* t,
                                float* const ns[3], float* const ng[3], hipStream_t st) {
    if (nq <= 0) return hipSuccess;
    if (mode == 0)
        hipLaunchKernelGGL(scene_shading_kernel<false>, grid_for(nq), dim3(256), 0, st, S, shade, nq, o[0], o[1],
                           o[2], d[0], d[1], d[2], mint, maxt, prim, t, ns[0], ns[1], ns[2], ng[0], ng[1], ng[2]);
    else
        hipLaunchKernelGGL(scene_shading_kernel<true>, grid_for(nq), dim3(256), 0, st, S, shade, nq, o[0], o[1],
                           o[2], d[0], d[1], d[2], mint, maxt, prim, t, ns[0], ns[1], ns[2], ng[0], ng[1], ng[2]);
    return hipGetLastError();
}

// sdmm_scene_texture: sdmm_scene_intersect's search, then the hit's uv and the
// effective reflectance of its BSDF as the Li kernels compute them (hit_uv,
// hit_reflectance); zeros on a miss
template <bool BRUTE>
__global__ void __launch_bounds__(256)
scene_texture_kernel(SceneDev S, TexDev T, int64_t nq, const float* __restrict__ o0, const float* __restrict__ o1,
                     const float* __restrict__ o2, const float* __restrict__ d0, const float* __restrict__ d1,
                     const float* __restrict__ d2, float mint, float maxt, int32_t* __restrict__ prim,
                     float* __restrict__ t_out, float* __restrict__ uv0, float* __restrict__ uv1,
                     float* __restrict__ r, float* __restrict__ g, float* __restrict__ b) {
    __shared__ int bvh_lds[BRUTE ? 1 : kBvhStack * 256];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const float o[3] = {o0[i], o1[i], o2[i]}, d[3] = {d0[i], d1[i], d2[i]};
    float t;
    int best = quads_closest(S.quads, S.n_quads, o, d, mint, maxt, t);
    if (S.n_tris > 0) {
        if (BRUTE) {
            mesh_brute(S.tris, S.n_tris, S.n_quads, o, d, mint, maxt, best, t);
        } else {
            LdsStack st{bvh_lds + threadIdx.x};
            bvh_closest(S.nodes, S.tris, S.n_quads, o, d, mint, maxt, best, t, st);
        }
    }
    float uv[2] = {0.0f, 0.0f}, rgb[3] = {0.0f, 0.0f, 0.0f};
    if (best >= 0) {
        if (best >= S.n_quads && !T.mesh_uv) {
            // a mesh with neither mesh_uvs nor textures has no per-triangle table: the winner is looked
            // for in the leaf-ordered array (this entry alone pays for that) and its test gives (u, v)
            for (int k = 0; k < S.n_tris; ++k) {
                if (S.tris[k].id != best - S.n_quads) continue;
                float tt, u, v;
                if (tri_intersect_uv(S.tris[k], o, d, &tt, &u, &v)) { uv[0] = u; uv[1] = v; }
                break;
            }
        } else {
            hit_uv(S.quads, S.n_quads, T.mesh_uv, best, o, d, uv);
        }
        const int qb = best >= S.n_quads ? S.hits[best - S.n_quads].bsdf : S.quads[best].bsdf;
        hit_reflectance<true>(S.refl, T.tex, T.bsdf_tex, qb, uv, rgb);
    }
    prim[i] = best;
    t_out[i] = t;
    uv0[i] = uv[0]; uv1[i] = uv[1];
    r[i] = rgb[0]; g[i] = rgb[1]; b[i] = rgb[2];
}
hipError_t launch_scene_texture(const SceneDev& S, const TexDev& T, int64_t nq, const float* const o[3],
                                const float* const d[3], float mint, float maxt, int mode, int32_t* prim, float* t,
                                float* const uv[2], float* const rgb[3], hipStream_t st) {
    if (nq <= 0) return hipSuccess;
    if (mode == 0)
        hipLaunchKernelGGL(scene_texture_kernel<false>, grid_for(nq), dim3(256), 0, st, S, T, nq, o[0], o[1], o[2],
                           d[0], d[1], d[2], mint, maxt, prim, t, uv[0], uv[1], rgb[0], rgb[1], rgb[2]);
    else
        hipLaunchKernelGGL(scene_texture_kernel<true>, grid_for(nq), dim3(256), 0, st, S, T, nq, o[0], o[1], o[2],
                           d[0], d[1], d[2], mint, maxt, prim, t, uv[0], uv[1], rgb[0], rgb[1], rgb[2]);
    return hipGetLastError();
}

hipError_t launch_li_film(const PathsDev& P, int64_t pix0, int64_t npix, int spp, int64_t plane, float* image,
                          float* image_sqr, hipStream_t st) {
    hipLaunchKernelGGL(li_film_kernel, grid_for(npix), dim3(256), 0, st, P, pix0, npix, spp, plane, image, image_sqr);
    return hipGetLastError();
}

size_t produce_temp_bytes(int64_t n_paths, int64_t n_records, int key_bits) {
    size_t a = 0, b = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, a, (const int64_t*)nullptr, (int64_t*)nullptr, (int)n_paths);
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                             (const int64_t*)nullptr, (int64_t*)nullptr, (int)n_records, 0,
                                             key_bits);
    return a > b ? a : b;
}

// count + scan: offsets[p] (n_paths + 1 entries; offsets[n_paths] = total)
hipError_t launch_produce_count(const STNodeDev* nodes, const PathsDev& P, int64_t path0, int saved, uint64_t seed,
                                int64_t* count, int64_t* offsets, void* temp, size_t temp_bytes, hipStream_t st) {
    hipLaunchKernelGGL(produce_count_kernel, grid_for(P.P), dim3(256), 0, st, nodes, P, path0, saved, seed,
                       count);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return hipcub::DeviceScan::ExclusiveSum(temp, temp_bytes, count, offsets, (int)P.P + 1, st);
}

hipError_t launch_produce_records(const STNodeDev* nodes, int num_nodes, int key_bits, const PathsDev& P,
                                  int64_t path0, int saved, uint64_t seed, const int64_t* offsets, int64_t n_rec,
                                  uint32_t* keys0, uint32_t* keys1, int64_t* codes0, int64_t* codes1, void* recs,
                                  void* temp, size_t temp_bytes, int64_t* seg_dev, int* lost, float* const x[6],
                                  float* const nrm[3], float* w, uint8_t* stats, int32_t* node, int64_t* source,
                                  hipStream_t st) {
    hipLaunchKernelGGL(produce_write_kernel, grid_for(P.P), dim3(256), 0, st, nodes, P, path0, saved, seed,
                       offsets, keys0, codes0, (ProducedRec*)recs, lost);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || n_rec == 0) return e;
    // stable: a leaf's records stay in (path, push) order
    e = hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, keys0, keys1, codes0, codes1, (int)n_rec, 0, key_bits,
                                           st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(produce_seg_kernel, grid_for(num_nodes + 1), dim3(256), 0, st, keys1, n_rec, num_nodes,
                       seg_dev);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(produce_gather_kernel, grid_for(n_rec), dim3(256), 0, st, (const ProducedRec*)recs, codes1,
                       n_rec, x[0], x[1], x[2],
                       x[3], x[4], x[5], nrm ? nrm[0] : nullptr, nrm ? nrm[1] : nullptr, nrm ? nrm[2] : nullptr, w,
                       stats, keys1, node, source);
    return hipGetLastError();
}

}  // namespace sdmm
