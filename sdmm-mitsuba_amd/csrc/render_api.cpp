// render_api.cpp -- host side of the device Li (render.hip) behind
// include/sdmm_gpu.h: the analytic scene, the per-bounce launch sequence
// (camera -> [query -> guided wavefront -> shade] x bounces -> film) and the
// path / query / vertex buffers, grown on demand and reused across renders.
#include <hip/hip_runtime.h>
#include <xmmintrin.h>

#include <hipcub/hipcub.hpp>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/sdmm_gpu.h"
#include "render_device.h"
#include "render_launch.h"
#include "host_xfer.h"
#include "learned_bsdf.h"
#include "bsdf_phong.h"
#include "bsdf_roughdielectric.h"
#include "bsdf_smooth.h"

// the scene's derived quad data in plain IEEE float (no FMA contraction), as
// the CPU restatement of Li forms it (oracle/sdmm_oracle_li.inc)
#pragma clang fp contract(off)

using namespace sdmm;

struct sdmm_scene {
    int device = 0;
    SceneDev S{};
    QuadDev* dquads = nullptr;
    float* drefl = nullptr;
    float* dbpar = nullptr;
    float* dlmod = nullptr;   // kLearnedStride per BSDF (learned_models), null: none
    float* dlmod_nd = nullptr;   // kLearnedNdStride per BSDF (learned_models_nd), null: none
    int32_t* dtwosided = nullptr;   // 1 per two-sided BSDF (bsdf_twosided), null: no entry set
    float* drad = nullptr;
    BvhNode* dnodes = nullptr;   // the triangle mesh (mesh_bvh.h), null without one
    MeshTri* dtris = nullptr;
    MeshHit* dhits = nullptr;
    MeshShade* dshade = nullptr;   // the mesh's vertex normals (shading_normal.h), null without them
    EnvTexel* denv = nullptr;    // the lat-long environment map (envmap.h), null without one
    float smin[3] = {0, 0, 0}, snorm = 1.0f, tmin[3] = {0, 0, 0}, tmax[3] = {0, 0, 0};
    // per-render buffers (grown)
    void* buf = nullptr;
    size_t buf_bytes = 0;
    int64_t cap_paths = 0;
    int cap_v = 0;
    PathsDev P{};
    QueryDev Q{};
    NormalsDev N{};   // (vertex normals: N.shade = dshade, the ns / ng planes in buf)
    int64_t* dsum = nullptr;
    int32_t* dcount = nullptr;   // live guided queries of the current bounce
    int32_t* hcount = nullptr;   // (pinned host copy)
    int32_t* hfb = nullptr;      // per bounce: fallback queries of its wavefront (pinned)
    int hfb_cap = 0;
    void* temp = nullptr;
    size_t temp_bytes = 0;
    // rough conductors / Phong BSDFs with product sampling: the extended
    // learned-BSDF table -- the caller's B rows re-strided to lM >= kLearnedKeep
    // lobes, then one row per compact query for the material's per-bounce lobes
    bool per_query_lobes = false;
    void* lt = nullptr;
    size_t lt_bytes = 0;
};

namespace {

int fail(int code, const std::string& m) { return sdmm_detail::set_error(code, m.c_str()); }

#define HIP_TRY(expr)                                                                     \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess)                                                             \
            return fail(SDMM_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));   \
    } while (0)

void cross3(const float a[3], const float b[3], float c[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
float dot3h(const float a[3], const float b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// path + query + vertex planes for P paths with V vertex slots
int grow(sdmm_scene* s, int64_t P, int V, hipStream_t st) {
    if (P <= s->cap_paths && V <= s->cap_v && s->buf) return SDMM_OK;
    const bool diel = s->S.has_dielectric != 0;   // (the eta planes: only with a dielectric or a kind-5 / 6 BSDF)
    const bool nrm = s->N.shade != nullptr;       // (the ns / ng planes: only with vertex normals)
    const int64_t cap = std::max<int64_t>(P, s->cap_paths);
    const int cv = std::max(V, s->cap_v);
    auto al = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t f = al(sizeof(float) * (size_t)cap), i4 = al(sizeof(int32_t) * (size_t)cap), u1 = al((size_t)cap);
    const size_t recb = al(sizeof(float) * (size_t)kVertexFields * (size_t)cv * (size_t)cap);
    size_t tb = 0;
    (void)hipcub::DeviceReduce::Sum(nullptr, tb, (const int32_t*)nullptr, (int64_t*)nullptr, (int)cap);
    tb = std::max(tb, li_select_temp_bytes(cap));
    const size_t need = 12 * f + 4 * i4 + recb + 13 * f + u1 + i4 + 256 + al(tb) + 9 * f + 2 * u1 + 3 * i4 +
                        (1 + 1 + 9 + 1) * f + i4 + u1 + 4 * f + (diel ? 2 * f : 0) + (nrm ? 6 * f : 0);
    HIP_TRY(hipStreamSynchronize(st));
    if (s->buf) HIP_TRY(hipFree(s->buf));
    s->buf = nullptr;
    HIP_TRY(hipMalloc(&s->buf, need));
    s->buf_bytes = need;
    s->cap_paths = cap;
    s->cap_v = cv;
    char* b = (char*)s->buf;
    auto take = [&](size_t n) { char* r = b; b += n; return r; };
    float** pf[12] = {&s->P.px, &s->P.py, &s->P.pz, &s->P.dx, &s->P.dy, &s->P.dz,
                      &s->P.tr, &s->P.tg, &s->P.tb, &s->P.lr, &s->P.lg, &s->P.lb};
    for (float** q : pf) *q = (float*)take(f);
    s->P.depth = (int*)take(i4);
    s->P.quad = (int*)take(i4);
    s->P.nv = (int*)take(i4);
    s->P.nray = (int*)take(i4);
    s->P.rec = (float*)take(recb);
    float** qf[13] = {&s->Q.c0, &s->Q.c1, &s->Q.c2, &s->Q.u0, &s->Q.u1, &s->Q.u2, &s->Q.b0,
                      &s->Q.b1, &s->Q.b2, &s->Q.d0, &s->Q.d1, &s->Q.d2, &s->Q.pdf};
    for (float** q : qf) *q = (float*)take(f);
    s->Q.mode = (uint8_t*)take(u1);
    s->Q.comp = (int32_t*)take(i4);
    s->dsum = (int64_t*)take(256);
    s->temp = take(al(tb));
    s->temp_bytes = al(tb);
    float** kf[9] = {&s->Q.k_c0, &s->Q.k_c1, &s->Q.k_c2, &s->Q.k_u0, &s->Q.k_u1, &s->Q.k_u2,
                     &s->Q.k_b0, &s->Q.k_b1, &s->Q.k_b2};
    for (float** q : kf) *q = (float*)take(f);
    s->Q.k_mode = (uint8_t*)take(u1);
    s->Q.live = (uint8_t*)take(u1);
    s->Q.idx = (int32_t*)take(i4);
    s->Q.slot = (int32_t*)take(i4);
    s->dcount = (int32_t*)take(i4);
    s->Q.ch = (float*)take(f);
    s->Q.k_ch = (float*)take(f);
    for (int i = 0; i < 9; ++i) s->Q.k_F[i] = (float*)take(f);
    s->Q.hq = (float*)take(f);
    s->Q.k_mat = (int32_t*)take(i4);
    s->Q.bdelta = (uint8_t*)take(u1);
    float** bf[4] = {&s->Q.bw0, &s->Q.bw1, &s->Q.bw2, &s->Q.bpdf};
    for (float** q : bf) *q = (float*)take(f);
    s->P.eta = diel ? (float*)take(f) : nullptr;
    s->Q.beta = diel ? (float*)take(f) : nullptr;
    float** nf[6] = {&s->N.nsx, &s->N.nsy, &s->N.nsz, &s->N.ngx, &s->N.ngy, &s->N.ngz};
    for (float** q : nf) *q = nrm ? (float*)take(f) : nullptr;
    return SDMM_OK;
}

// The extended learned-BSDF table of a render with rough conductors or Phong
// BSDFs (the materials that condition a learned model per bounce): rows
// 0 .. B-1 the caller's (device arrays, re-strided to lM = max(M,
// kLearnedKeep) lobes, the extra lobes weight 0 -- skipped by the product),
// rows B .. B + cap - 1 the compact queries' own lobes (written by
// li_compact_kernel; hence the component index k * max(M, 2) + j of such a
// render).  *tab describes it; s->Q points at the query rows.
int extend_learned(sdmm_scene* s, const sdmm_bsdf_table& user, int64_t cap, hipStream_t st, sdmm_bsdf_table* tab) {
    const int M = user.M, lM = std::max(M, kLearnedKeep), B = user.B;
    const int64_t rows = (int64_t)B + cap;
    auto al = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t wb = al(sizeof(float) * (size_t)rows * lM), mb = 3 * wb, cb = 4 * wb, db = al((size_t)rows);
    const size_t need = wb + mb + cb + db;
    if (need > s->lt_bytes) {
        HIP_TRY(hipStreamSynchronize(st));
        if (s->lt) HIP_TRY(hipFree(s->lt));
        s->lt = nullptr;
        s->lt_bytes = 0;
        HIP_TRY(hipMalloc(&s->lt, need));
        s->lt_bytes = need;
    }
    char* b = (char*)s->lt;
    float* w = (float*)b;
    float* m = (float*)(b + wb);
    float* c = (float*)(b + wb + mb);
    uint8_t* dflag = (uint8_t*)(b + wb + mb + cb);
    HIP_TRY(hipMemsetAsync(w, 0, sizeof(float) * (size_t)B * lM, st));
    HIP_TRY(hipMemcpy2DAsync(w, sizeof(float) * lM, user.weights, sizeof(float) * M, sizeof(float) * M, B,
                             hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemsetAsync(m, 0, sizeof(float) * 3 * (size_t)B * lM, st));
    HIP_TRY(hipMemcpy2DAsync(m, sizeof(float) * 3 * lM, user.means, sizeof(float) * 3 * M, sizeof(float) * 3 * M, B,
                             hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemsetAsync(c, 0, sizeof(float) * 4 * (size_t)B * lM, st));
    HIP_TRY(hipMemcpy2DAsync(c, sizeof(float) * 4 * lM, user.covs, sizeof(float) * 4 * M, sizeof(float) * 4 * M, B,
                             hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemsetAsync(dflag, 0, (size_t)rows, st));
    if (user.diffuse) HIP_TRY(hipMemcpyAsync(dflag, user.diffuse, (size_t)B, hipMemcpyDeviceToDevice, st));
    *tab = sdmm_bsdf_table{w, m, c, (int)std::min<int64_t>(rows, INT32_MAX), lM, dflag};
    s->Q.lw = w;
    s->Q.lm = m;
    s->Q.lc = c;
    s->Q.lrow0 = B;
    s->Q.lM = lM;
    return SDMM_OK;
}

// the geometry and material arguments of a description (sdmm_scene_create
// and the host intersect entry): some primitive, its arrays, a BSDF table
bool geometry_args_ok(const sdmm_scene_desc* d) {
    return d->n_quads >= 0 && d->n_triangles >= 0 && (d->n_quads > 0 || d->n_triangles > 0) &&
           (d->n_quads == 0 || (d->quads && d->bsdf)) && d->n_bsdfs >= 1 && d->reflectance;
}
// some primitive may carry an emitter index (quads' or triangles' array set):
// the radiance table is needed, uploaded and read then
bool has_emitters(const sdmm_scene_desc* d) { return d->emitter || (d->n_triangles > 0 && d->tri_emitter); }

// the description's environment emitter, validated; *E gets every field but
// the texel pointer.  0, or the error code (message set).
int prep_env(const sdmm_scene_desc* d, const char* who, EnvDev* E) {
    const std::string w(who);
    *E = EnvDev{};
    if (d->env_kind < kEnvNone || d->env_kind > kEnvLatLong)
        return fail(SDMM_E_INVALID, w + ": env_kind outside 0..2");
    E->kind = d->env_kind;
    if (d->env_kind == kEnvConstant) {
        for (int c = 0; c < 3; ++c) {
            if (!(std::isfinite(d->env_radiance[c]) && d->env_radiance[c] >= 0.0f))
                return fail(SDMM_E_INVALID, w + ": a non-finite or negative env_radiance");
            E->rad[c] = d->env_radiance[c];
        }
    } else if (d->env_kind == kEnvLatLong) {
        if (!d->env_pixels) return fail(SDMM_E_INVALID, w + ": a lat-long environment without env_pixels");
        if (d->env_width < 1 || d->env_height < 1)
            return fail(SDMM_E_INVALID, w + ": env_width or env_height < 1");
        const int64_t n = (int64_t)d->env_width * d->env_height;
        if (n > kEnvMaxTexels) return fail(SDMM_E_INVALID, w + ": an environment map of more than 2^26 texels");
        if (!(std::isfinite(d->env_scale) && d->env_scale >= 0.0f))
            return fail(SDMM_E_INVALID, w + ": a non-finite or negative env_scale");
        for (int i = 0; i < 9; ++i)
            if (!std::isfinite(d->env_world_to_local[i]))
                return fail(SDMM_E_INVALID, w + ": a non-finite env_world_to_local entry");
        for (int64_t i = 0; i < 3 * n; ++i)
            if (!(std::isfinite(d->env_pixels[i]) && d->env_pixels[i] >= 0.0f))
                return fail(SDMM_E_INVALID, w + ": a non-finite or negative environment texel");
        E->w = d->env_width;
        E->h = d->env_height;
        E->scale = d->env_scale;
        for (int i = 0; i < 9; ++i) E->m[i] = d->env_world_to_local[i];
    }
    return SDMM_OK;
}

// the description's two-sided flags, validated (after geometry_args_ok); *any
// (nullable): some entry is set.  0, or the error code (message set).
int prep_twosided(const sdmm_scene_desc* d, const char* who, bool* any) {
    const std::string w(who);
    if (any) *any = false;
    if (!d->bsdf_twosided) return SDMM_OK;
    for (int b = 0; b < d->n_bsdfs; ++b) {
        const int32_t v = d->bsdf_twosided[b];
        if (v != 0 && v != 1) return fail(SDMM_E_INVALID, w + ": a bsdf_twosided entry other than 0 or 1");
        if (v == 0) continue;
        // "Only materials without a transmission component can be nested" (twosided.cpp:106-108)
        const float kind = d->bsdf_params ? d->bsdf_params[kBsdfParams * b] : (float)kBsdfDiffuse;
        if (kind == (float)kBsdfDielectric || kind == (float)kBsdfSmoothDielectric)
            return fail(SDMM_E_INVALID, w + ": bsdf_twosided on a transmitting BSDF (kind 4 or 5)");
        if (any) *any = true;
    }
    return SDMM_OK;
}

// the quads' derived data (normal, duals) and their corners' AABB, after the
// description's argument checks.  0, or the error code (message set).
int prep_quads(const sdmm_scene_desc* d, const char* who, std::vector<QuadDev>* qs, float mn[3], float mx[3]) {
    const std::string w(who);
    if (!geometry_args_ok(d)) return fail(SDMM_E_INVALID, w + ": invalid description");
    if (d->mesh_normals && d->n_triangles < 1) return fail(SDMM_E_INVALID, w + ": mesh_normals without triangles");
    if (const int rc = prep_twosided(d, who, nullptr)) return rc;
    if (has_emitters(d) && (d->n_emitters < 1 || !d->radiance))
        return fail(SDMM_E_INVALID, w + ": emitters without radiance");
    qs->assign((size_t)d->n_quads, QuadDev{});
    for (int q = 0; q < d->n_quads; ++q) {
        QuadDev& Q = (*qs)[(size_t)q];
        const float* v = d->quads + 9 * q;
        for (int a = 0; a < 3; ++a) { Q.p0[a] = v[a]; Q.e1[a] = v[3 + a]; Q.e2[a] = v[6 + a]; }
        float n[3];
        cross3(Q.e1, Q.e2, n);
        const float len = std::sqrt(dot3h(n, n));
        if (!(len > 0.0f)) return fail(SDMM_E_INVALID, w + ": degenerate quad");
        const float sg = (d->flip_normals && d->flip_normals[q]) ? -1.0f : 1.0f;
        for (int a = 0; a < 3; ++a) Q.n[a] = sg * n[a] / len;
        // duals: g1 . e1 = 1, g1 . e2 = 0 (g1 ~ e2 x n), likewise g2
        float a1[3], a2[3];
        cross3(Q.e2, n, a1);
        cross3(n, Q.e1, a2);
        const float s1 = dot3h(Q.e1, a1), s2 = dot3h(Q.e2, a2);
        for (int a = 0; a < 3; ++a) { Q.g1[a] = a1[a] / s1; Q.g2[a] = a2[a] / s2; }
        Q.bsdf = d->bsdf[q];
        Q.emitter = d->emitter ? d->emitter[q] : -1;
        if (Q.bsdf < 0 || Q.bsdf >= d->n_bsdfs || Q.emitter < -1 || (Q.emitter >= 0 && Q.emitter >= d->n_emitters))
            return fail(SDMM_E_INVALID, w + ": material index out of range");
        // scene AABB without the camera: the four corners
        for (int c = 0; c < 4; ++c)
            for (int a = 0; a < 3; ++a) {
                const float x = Q.p0[a] + ((c & 1) ? Q.e1[a] : 0.0f) + ((c & 2) ? Q.e2[a] : 0.0f);
                mn[a] = std::min(mn[a], x);
                mx[a] = std::max(mx[a], x);
            }
    }
    return SDMM_OK;
}

// the description's triangle mesh, validated and built (n_triangles > 0);
// max_levels 0: the traversal stack's cap
int prep_mesh(const sdmm_scene_desc* d, const char* who, int max_levels, MeshBvh* m) {
    MeshInput in;
    in.n_vertices = d->n_mesh_vertices;
    in.vertices = d->mesh_vertices;
    in.n_triangles = d->n_triangles;
    in.triangles = d->triangles;
    in.bsdf = d->tri_bsdf;
    in.emitter = d->tri_emitter;
    in.flip = d->tri_flip_normals;
    in.normals = d->mesh_normals;
    in.n_bsdfs = d->n_bsdfs;
    in.n_emitters = d->n_emitters;
    std::string err;
    if (!mesh_build(in, max_levels, m, &err)) return fail(SDMM_E_INVALID, std::string(who) + ": " + err);
    return SDMM_OK;
}

}  // namespace

extern "C" {

int sdmm_scene_create(const sdmm_scene_desc* d, int device, sdmm_scene** out) {
    if (!out || !d || !geometry_args_ok(d) || d->width < 1 || d->height < 1 ||
        !(d->fov_x_deg > 0.0f && d->fov_x_deg < 180.0f))
        return fail(SDMM_E_INVALID, "sdmm_scene_create: invalid description");
    if (has_emitters(d) && (d->n_emitters < 1 || !d->radiance))
        return fail(SDMM_E_INVALID, "sdmm_scene_create: emitters without radiance");
    if (d->bsdf_params)
        for (int b = 0; b < d->n_bsdfs; ++b) {
            const float* bp = d->bsdf_params + kBsdfParams * b;
            const bool ok = bp[0] == (float)kBsdfDiffuse ||
                            (bp[0] == (float)kBsdfPlastic && bp[4] > 0.0f && bp[5] > 0.0f && bp[6] < 1.0f &&
                             bp[7] >= 0.0f && bp[7] <= 1.0f) ||
                            (bp[0] == (float)kBsdfConductor && bp[1] >= 0.0f && bp[2] >= 0.0f && bp[3] >= 0.0f &&
                             std::isfinite(bp[1] + bp[2] + bp[3]) && bp[4] > 0.0f && std::isfinite(bp[4]) &&
                             bp[5] >= 0.0f && std::isfinite(bp[5]) && bp[6] > 0.0f && bp[6] <= 2.0f) ||
                            (bp[0] == (float)kBsdfPhong && bp[1] >= 0.0f && bp[2] >= 0.0f && bp[3] >= 0.0f &&
                             std::isfinite(bp[1] + bp[2] + bp[3]) && bp[4] >= 0.0f && std::isfinite(bp[4]) &&
                             bp[5] >= 0.0f && bp[5] <= 1.0f) ||
                            (bp[0] == (float)kBsdfDielectric && bp[1] >= 0.0f && bp[2] >= 0.0f && bp[3] >= 0.0f &&
                             std::isfinite(bp[1] + bp[2] + bp[3]) && bp[4] > 0.0f && bp[4] != 1.0f &&
                             std::isfinite(bp[4]) && bp[5] > 0.0f && std::isfinite(bp[5]) && bp[6] > 0.0f &&
                             bp[6] <= 2.0f) ||
                            (bp[0] == (float)kBsdfSmoothDielectric && bp[1] >= 0.0f && bp[2] >= 0.0f &&
                             bp[3] >= 0.0f && std::isfinite(bp[1] + bp[2] + bp[3]) && bp[4] > 0.0f &&
                             bp[4] != 1.0f && std::isfinite(bp[4]) && bp[5] > 0.0f && std::isfinite(bp[5])) ||
                            (bp[0] == (float)kBsdfSmoothConductor && bp[1] >= 0.0f && bp[2] >= 0.0f &&
                             bp[3] >= 0.0f && std::isfinite(bp[1] + bp[2] + bp[3]) && bp[4] > 0.0f &&
                             std::isfinite(bp[4]) && bp[5] >= 0.0f && std::isfinite(bp[5]));
            if (!ok) return fail(SDMM_E_INVALID, "sdmm_scene_create: invalid bsdf_params");
            // a smooth dielectric's specularTransmittance (its reflectance row)
            const float* tr = d->reflectance + 3 * b;
            if (bp[0] == (float)kBsdfSmoothDielectric &&
                !(tr[0] >= 0.0f && tr[1] >= 0.0f && tr[2] >= 0.0f && std::isfinite(tr[0] + tr[1] + tr[2])))
                return fail(SDMM_E_INVALID, "sdmm_scene_create: invalid bsdf_params (a smooth dielectric's "
                                            "transmittance is negative or not finite)");
        }
    // learned models: at most kLearnedMaxComp components, finite, unit directions
    std::vector<float> lmod;
    if (d->learned_models) {
        lmod.assign((size_t)kLearnedStride * (size_t)d->n_bsdfs, 0.0f);
        for (int b = 0; b < d->n_bsdfs; ++b) {
            const sdmm_learned_bsdf4& L = d->learned_models[b];
            if (L.M == 0) continue;
            // (a delta-only BSDF never calls getDMM: its entry is not read, not even checked)
            if (d->bsdf_params && is_smooth_kind(d->bsdf_params[kBsdfParams * b])) continue;
            if (L.M < 0 || L.M > kLearnedMaxComp || !L.weights || !L.means || !L.covs)
                return fail(SDMM_E_INVALID, "sdmm_scene_create: invalid learned model (1 <= M <= 8, arrays)");
            float* o = lmod.data() + (size_t)kLearnedStride * b;
            o[0] = (float)L.M;
            for (int k = 0; k < L.M; ++k) {
                float* r = o + 1 + kLearnedRec * k;
                r[0] = L.weights[k];
                for (int i = 0; i < 5; ++i) r[1 + i] = L.means[5 * k + i];
                for (int i = 0; i < 16; ++i) r[6 + i] = L.covs[16 * k + i];
                bool ok = r[0] >= 0.0f;
                for (int i = 0; i < kLearnedRec; ++i) ok = ok && std::isfinite(r[i]);
                const double n2 = (double)r[3] * r[3] + (double)r[4] * r[4] + (double)r[5] * r[5];
                if (!ok || std::fabs(n2 - 1.0) > 1e-5)
                    return fail(SDMM_E_INVALID, "sdmm_scene_create: learned model with a non-finite value, a "
                                                "negative weight or a non-unit direction");
            }
        }
    }
    // learned models over a C-dimensional condition: the same checks; a Phong
    // BSDF's is its SDMM5 with the forced diffuse component 1, a rough
    // dielectric's its SDMM5 over (theta_i, alpha, eta)
    std::vector<float> lmod_nd;
    if (d->learned_models_nd) {
        lmod_nd.assign((size_t)kLearnedNdStride * (size_t)d->n_bsdfs, 0.0f);
        for (int b = 0; b < d->n_bsdfs; ++b) {
            const sdmm_learned_bsdf& L = d->learned_models_nd[b];
            if (L.M == 0) continue;
            if (d->bsdf_params && is_smooth_kind(d->bsdf_params[kBsdfParams * b])) continue;   // (as above)
            if ((L.C != 2 && L.C != 3) || L.M < 0 || L.M > kLearnedMaxComp || !L.weights || !L.means || !L.covs)
                return fail(SDMM_E_INVALID, "sdmm_scene_create: invalid learned model (C 2 or 3, 1 <= M <= 8, arrays)");
            const bool phong = d->bsdf_params && d->bsdf_params[kBsdfParams * b] == (float)kBsdfPhong;
            if (phong && (L.C != 3 || L.M <= kPhongDiffuseComponent))
                return fail(SDMM_E_INVALID, "sdmm_scene_create: a Phong BSDF's learned model needs C = 3 and M >= 2");
            const bool diel = d->bsdf_params && d->bsdf_params[kBsdfParams * b] == (float)kBsdfDielectric;
            if (diel && L.C != 3)
                return fail(SDMM_E_INVALID, "sdmm_scene_create: a rough dielectric's learned model needs C = 3");
            const int R = learned_rec(L.C), nm = L.C + 3, nc = (L.C + 2) * (L.C + 2);
            float* o = lmod_nd.data() + (size_t)kLearnedNdStride * b;
            o[0] = (float)L.C;
            o[1] = (float)L.M;
            for (int k = 0; k < L.M; ++k) {
                float* r = o + 2 + R * k;
                r[0] = L.weights[k];
                for (int i = 0; i < nm; ++i) r[1 + i] = L.means[nm * k + i];
                for (int i = 0; i < nc; ++i) r[1 + nm + i] = L.covs[nc * k + i];
                bool ok = r[0] >= 0.0f;
                for (int i = 0; i < R; ++i) ok = ok && std::isfinite(r[i]);
                const float* dir = r + 1 + L.C;
                const double n2 = (double)dir[0] * dir[0] + (double)dir[1] * dir[1] + (double)dir[2] * dir[2];
                if (!ok || std::fabs(n2 - 1.0) > 1e-5)
                    return fail(SDMM_E_INVALID, "sdmm_scene_create: learned model with a non-finite value, a "
                                                "negative weight or a non-unit direction");
            }
        }
    }
    *out = nullptr;
    std::vector<QuadDev> qs;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    int rc = prep_quads(d, "sdmm_scene_create", &qs, mn, mx);
    if (rc) return rc;
    bool twosided = false;   // (validated in prep_quads; all zeros: no device table)
    rc = prep_twosided(d, "sdmm_scene_create", &twosided);
    if (rc) return rc;
    // the triangle mesh: validated, its BVH built; the AABB takes its vertices in
    MeshBvh mesh;
    if (d->n_triangles > 0) {
        rc = prep_mesh(d, "sdmm_scene_create", 0, &mesh);
        if (rc) return rc;
        for (int a = 0; a < 3; ++a) {
            mn[a] = std::min(mn[a], mesh.mn[a]);
            mx[a] = std::max(mx[a], mesh.mx[a]);
        }
    }
    // the environment emitter: validated, a lat-long map as RGBA texels (envmap.h)
    EnvDev env;
    rc = prep_env(d, "sdmm_scene_create", &env);
    if (rc) return rc;
    std::vector<EnvTexel> env_texels;
    if (env.kind == kEnvLatLong) {
        env_texels.resize((size_t)env.w * (size_t)env.h);
        for (size_t i = 0; i < env_texels.size(); ++i)
            env_texels[i] = EnvTexel{d->env_pixels[3 * i], d->env_pixels[3 * i + 1], d->env_pixels[3 * i + 2], 0.0f};
    }
    sdmm_scene* s = new (std::nothrow) sdmm_scene();
    if (!s) return fail(SDMM_E_NOMEM, "out of host memory");
    s->device = device;
    // (a conductor some quad uses: the CPU restatement's rule)
    if (d->bsdf_params)
        for (int q = 0; q < d->n_quads; ++q)
            if (d->bsdf_params[kBsdfParams * d->bsdf[q]] == (float)kBsdfConductor ||
                d->bsdf_params[kBsdfParams * d->bsdf[q]] == (float)kBsdfPhong ||
                d->bsdf_params[kBsdfParams * d->bsdf[q]] == (float)kBsdfDielectric)
                s->per_query_lobes = true;
    if (d->bsdf_params)
        for (int i = 0; i < d->n_triangles; ++i) {
            const float kind = d->bsdf_params[kBsdfParams * d->tri_bsdf[i]];
            if (kind == (float)kBsdfConductor || kind == (float)kBsdfPhong || kind == (float)kBsdfDielectric)
                s->per_query_lobes = true;
        }
    // render() (volpath_sdmm.cpp:375-393): spatialNormalization = the largest
    // extent; the tree box getAABB (:314-332)
    float ext[3], norm = 0.0f;
    for (int a = 0; a < 3; ++a) { ext[a] = mx[a] - mn[a]; norm = std::max(norm, ext[a]); }
    for (int a = 0; a < 3; ++a) {
        s->smin[a] = mn[a];
        s->tmin[a] = 0.0f - 1e-5f;
        s->tmax[a] = ext[a] / norm + 1e-5f;
    }
    s->snorm = norm;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipMalloc(&s->dquads, sizeof(QuadDev) * std::max<size_t>(qs.size(), 1));
    if (e == hipSuccess && d->n_triangles > 0) e = hipMalloc(&s->dnodes, sizeof(BvhNode) * mesh.nodes.size());
    if (e == hipSuccess && d->n_triangles > 0) e = hipMalloc(&s->dtris, sizeof(MeshTri) * mesh.tris.size());
    if (e == hipSuccess && d->n_triangles > 0) e = hipMalloc(&s->dhits, sizeof(MeshHit) * mesh.hits.size());
    if (e == hipSuccess && d->n_triangles > 0)
        e = hipMemcpy(s->dnodes, mesh.nodes.data(), sizeof(BvhNode) * mesh.nodes.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess && d->n_triangles > 0)
        e = hipMemcpy(s->dtris, mesh.tris.data(), sizeof(MeshTri) * mesh.tris.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess && d->n_triangles > 0)
        e = hipMemcpy(s->dhits, mesh.hits.data(), sizeof(MeshHit) * mesh.hits.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess && !mesh.shade.empty()) e = hipMalloc(&s->dshade, sizeof(MeshShade) * mesh.shade.size());
    if (e == hipSuccess && !mesh.shade.empty())
        e = hipMemcpy(s->dshade, mesh.shade.data(), sizeof(MeshShade) * mesh.shade.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess && !env_texels.empty()) e = hipMalloc(&s->denv, sizeof(EnvTexel) * env_texels.size());
    if (e == hipSuccess && !env_texels.empty())
        e = hipMemcpy(s->denv, env_texels.data(), sizeof(EnvTexel) * env_texels.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc(&s->drefl, sizeof(float) * 3 * (size_t)d->n_bsdfs);
    if (e == hipSuccess && has_emitters(d)) e = hipMalloc(&s->drad, sizeof(float) * 3 * (size_t)d->n_emitters);
    if (e == hipSuccess && d->bsdf_params)
        e = hipMalloc(&s->dbpar, sizeof(float) * kBsdfParams * (size_t)d->n_bsdfs);
    if (e == hipSuccess && d->bsdf_params)
        e = hipMemcpy(s->dbpar, d->bsdf_params, sizeof(float) * kBsdfParams * (size_t)d->n_bsdfs,
                      hipMemcpyHostToDevice);
    if (e == hipSuccess && !lmod.empty()) e = hipMalloc(&s->dlmod, sizeof(float) * lmod.size());
    if (e == hipSuccess && !lmod.empty())
        e = hipMemcpy(s->dlmod, lmod.data(), sizeof(float) * lmod.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess && !lmod_nd.empty()) e = hipMalloc(&s->dlmod_nd, sizeof(float) * lmod_nd.size());
    if (e == hipSuccess && !lmod_nd.empty())
        e = hipMemcpy(s->dlmod_nd, lmod_nd.data(), sizeof(float) * lmod_nd.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess && twosided) e = hipMalloc(&s->dtwosided, sizeof(int32_t) * (size_t)d->n_bsdfs);
    if (e == hipSuccess && twosided)
        e = hipMemcpy(s->dtwosided, d->bsdf_twosided, sizeof(int32_t) * (size_t)d->n_bsdfs, hipMemcpyHostToDevice);
    if (e == hipSuccess && !qs.empty())
        e = hipMemcpy(s->dquads, qs.data(), sizeof(QuadDev) * qs.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = hipMemcpy(s->drefl, d->reflectance, sizeof(float) * 3 * (size_t)d->n_bsdfs, hipMemcpyHostToDevice);
    if (e == hipSuccess && has_emitters(d))
        e = hipMemcpy(s->drad, d->radiance, sizeof(float) * 3 * (size_t)d->n_emitters, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        sdmm_scene_destroy(s);
        return fail(SDMM_E_HIP, std::string("sdmm_scene_create: ") + hipGetErrorString(e));
    }
    SceneDev& S = s->S;
    S.quads = s->dquads;
    S.n_quads = d->n_quads;
    S.refl = s->drefl;
    S.bpar = s->dbpar;
    S.lmodel = s->dlmod;
    S.lmodel_nd = s->dlmod_nd;
    S.twosided = s->dtwosided;
    S.nodes = s->dnodes;
    S.tris = s->dtris;
    S.hits = s->dhits;
    s->N.shade = s->dshade;
    S.n_tris = d->n_triangles;
    S.has_mesh = d->n_triangles > 0 ? 1 : 0;
    {
        // SDMM_MESH_BRUTE=1: the Li kernels loop over every triangle instead of walking the BVH (A/B)
        const char* ev = std::getenv("SDMM_MESH_BRUTE");
        S.mesh_brute = (ev && ev[0] == '1' && ev[1] == 0) ? 1 : 0;
    }
    if (d->bsdf_params)
        for (int b = 0; b < d->n_bsdfs; ++b) {
            if (d->bsdf_params[kBsdfParams * b] == (float)kBsdfPhong) S.has_phong = 1;
            if (d->bsdf_params[kBsdfParams * b] == (float)kBsdfDielectric) S.has_dielectric = 1;
            // (the delta-only kinds live in the DIEL kernels: no variant of their own)
            if (is_smooth_kind(d->bsdf_params[kBsdfParams * b])) S.has_dielectric = 1;
        }
    S.rad = s->drad;
    S.env = env;
    S.env.texels = reinterpret_cast<const float*>(s->denv);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) S.cam[4 * r + c] = d->camera_to_world[4 * r + c];
    S.tanx = (float)std::tan(0.5 * (double)d->fov_x_deg * 3.14159265358979323846 / 180.0);
    S.aspect = (float)d->width / (float)d->height;
    S.near_clip = d->near_clip > 0.0f ? d->near_clip : 1e-2f;
    S.width = d->width;
    S.height = d->height;
    for (int a = 0; a < 3; ++a) S.smin[a] = s->smin[a];
    S.snorm = s->snorm;
    *out = s;
    return SDMM_OK;
}

int sdmm_learned4_conditional(const sdmm_learned_bsdf4* m, float alpha, const float wi_local[3], int keep,
                              int* n_out, float* weights, float* means, float* covs) {
    if (!m || !wi_local || !n_out || keep < 1 || m->M < 0 || m->M > kLearnedMaxComp ||
        (m->M > 0 && (!m->weights || !m->means || !m->covs)) || !weights || !means || !covs)
        return fail(SDMM_E_INVALID, "sdmm_learned4_conditional: invalid argument");
    *n_out = 0;
    if (m->M == 0 || !(wi_local[2] > 0.0f)) return SDMM_OK;   // getDMM: no model, or cosTheta(wi) <= 0
    float rec[kLearnedMaxComp * kLearnedRec];
    for (int k = 0; k < m->M; ++k) {
        float* r = rec + kLearnedRec * k;
        r[0] = m->weights[k];
        for (int i = 0; i < 5; ++i) r[1 + i] = m->means[5 * k + i];
        for (int i = 0; i < 16; ++i) r[6 + i] = m->covs[16 * k + i];
    }
    // the device's float environment: denormals flushed (-fgpu-flush-denormals-to-zero)
    const unsigned csr = _mm_getcsr();
    _mm_setcsr(csr | 0x8040u);
    const float theta = (float)std::acos((double)std::fmin(1.0f, wi_local[2]));
    float w[kLearnedMaxComp], mm[3 * kLearnedMaxComp], cc[4 * kLearnedMaxComp];
    const int n = learned4_conditional(rec, m->M, theta, alpha, wi_local, keep, w, mm, cc);
    _mm_setcsr(csr);
    for (int j = 0; j < n; ++j) {
        weights[j] = w[j];
        for (int i = 0; i < 3; ++i) means[3 * j + i] = mm[3 * j + i];
        for (int i = 0; i < 4; ++i) covs[4 * j + i] = cc[4 * j + i];
    }
    *n_out = n;
    return SDMM_OK;
}

int sdmm_learned4_conditional_device(const sdmm_learned_bsdf4* m, float alpha, int64_t nq, const float* const wi_local[3],
                                     int keep, float* weights, float* means, float* covs, int32_t* n_out,
                                     void* hip_stream) {
    if (!m || nq < 0 || keep < 1 || keep > kLearnedMaxComp || m->M < 0 || m->M > kLearnedMaxComp ||
        (m->M > 0 && (!m->weights || !m->means || !m->covs)))
        return fail(SDMM_E_INVALID, "sdmm_learned4_conditional_device: invalid argument");
    if (nq == 0) return SDMM_OK;
    if (!wi_local || !wi_local[0] || !wi_local[1] || !wi_local[2] || !weights || !means || !covs || !n_out)
        return fail(SDMM_E_INVALID, "sdmm_learned4_conditional_device: invalid argument");
    float rec[kLearnedMaxComp * kLearnedRec];
    for (int k = 0; k < m->M; ++k) {
        float* r = rec + kLearnedRec * k;
        r[0] = m->weights[k];
        for (int i = 0; i < 5; ++i) r[1 + i] = m->means[5 * k + i];
        for (int i = 0; i < 16; ++i) r[6 + i] = m->covs[16 * k + i];
    }
    HIP_TRY(launch_learned4(rec, m->M, alpha, nq, wi_local, keep, weights, means, covs, n_out,
                            (hipStream_t)hip_stream));
    return SDMM_OK;
}

namespace {
// the model's records (learned_rec(C) floats each) from the ABI arrays
bool pack_learned(const sdmm_learned_bsdf* m, float* rec) {
    if (!m || (m->C != 2 && m->C != 3) || m->M < 0 || m->M > kLearnedMaxComp ||
        (m->M > 0 && (!m->weights || !m->means || !m->covs)))
        return false;
    const int R = learned_rec(m->C), nm = m->C + 3, nc = (m->C + 2) * (m->C + 2);
    for (int k = 0; k < m->M; ++k) {
        float* r = rec + R * k;
        r[0] = m->weights[k];
        for (int i = 0; i < nm; ++i) r[1 + i] = m->means[nm * k + i];
        for (int i = 0; i < nc; ++i) r[1 + nm + i] = m->covs[nc * k + i];
    }
    return true;
}
}  // namespace

int sdmm_learned_conditional(const sdmm_learned_bsdf* m, const float* cond_rest, const float wi_local[3], int keep,
                             int force, int* n_out, float* weights, float* means, float* covs) {
    float rec[kLearnedMaxComp * learned_rec(kLearnedMaxCond)];
    if (!pack_learned(m, rec) || !cond_rest || !wi_local || !n_out || keep < 0 || keep > kLearnedMaxComp ||
        force < -1 || force >= m->M || !weights || !means || !covs)
        return fail(SDMM_E_INVALID, "sdmm_learned_conditional: invalid argument (C 2 or 3, M <= 8, 0 <= keep <= 8, "
                                    "-1 <= force < M)");
    *n_out = 0;
    if (m->M == 0 || !(wi_local[2] > 0.0f)) return SDMM_OK;   // getDMM: no model, or cosTheta(wi) <= 0
    // the device's float environment: denormals flushed (-fgpu-flush-denormals-to-zero)
    const unsigned csr = _mm_getcsr();
    _mm_setcsr(csr | 0x8040u);
    float x[kLearnedMaxCond];
    x[0] = (float)std::acos((double)std::fmin(1.0f, wi_local[2]));
    for (int i = 0; i < m->C - 1; ++i) x[1 + i] = cond_rest[i];
    float w[kLearnedMaxComp], mm[3 * kLearnedMaxComp], cc[4 * kLearnedMaxComp];
    const int n = m->C == 2 ? learned_conditional<2>(rec, m->M, x, wi_local, keep, force, w, mm, cc)
                            : learned_conditional<3>(rec, m->M, x, wi_local, keep, force, w, mm, cc);
    _mm_setcsr(csr);
    for (int j = 0; j < n; ++j) {
        weights[j] = w[j];
        for (int i = 0; i < 3; ++i) means[3 * j + i] = mm[3 * j + i];
        for (int i = 0; i < 4; ++i) covs[4 * j + i] = cc[4 * j + i];
    }
    *n_out = n;
    return SDMM_OK;
}

int sdmm_learned_conditional_device(const sdmm_learned_bsdf* m, const float* const* cond_rest,
                                    const float* cond_scalar, int64_t nq, const float* const wi_local[3], int keep,
                                    int force, float* weights, float* means, float* covs, int32_t* n_out,
                                    void* hip_stream) {
    float rec[kLearnedMaxComp * learned_rec(kLearnedMaxCond)];
    if (!pack_learned(m, rec) || nq < 0 || keep < 0 || keep > kLearnedMaxComp || force < -1 ||
        force >= m->M)
        return fail(SDMM_E_INVALID, "sdmm_learned_conditional_device: invalid argument (C 2 or 3, M <= 8, 0 <= keep "
                                    "<= 8, -1 <= force < M)");
    if (nq == 0) return SDMM_OK;
    if (!wi_local || !wi_local[0] || !wi_local[1] || !wi_local[2] || !weights || !means || !covs || !n_out)
        return fail(SDMM_E_INVALID, "sdmm_learned_conditional_device: invalid argument");
    // every condition value comes from a plane or from a scalar
    for (int i = 0; i < m->C - 1; ++i)
        if (!(cond_rest && cond_rest[i]) && !cond_scalar)
            return fail(SDMM_E_INVALID, "sdmm_learned_conditional_device: a condition value with neither a plane "
                                        "nor a scalar");
    HIP_TRY(launch_learned_nd(m->C, rec, m->M, cond_rest, cond_scalar, nq, wi_local, keep, force, weights, means,
                              covs, n_out, (hipStream_t)hip_stream));
    return SDMM_OK;
}

int sdmm_bsdf_phong_host(const float* params, const float rho[3], const float wi[3], const float* u, float wo[3],
                         float value[3], float* pdf) {
    if (!params || params[0] != (float)kBsdfPhong || !rho || !wi || !wo || !value || !pdf)
        return fail(SDMM_E_INVALID, "sdmm_bsdf_phong_host: invalid argument (params of a kind-3 BSDF)");
    const unsigned csr = _mm_getcsr();
    _mm_setcsr(csr | 0x8040u);
    if (u) {
        float o[3] = {0.0f, 0.0f, 1.0f};
        phong_sample(wi, params, rho, u[0], u[1], o, value, pdf);
        for (int a = 0; a < 3; ++a) wo[a] = o[a];
    } else {
        *pdf = phong_eval_pdf(wi, wo, params, rho, value);
    }
    _mm_setcsr(csr);
    return SDMM_OK;
}

int sdmm_bsdf_roughdielectric_host(const float* params, const float spec_trans[3], const float wi[3], const float* u,
                                   float wo[3], float value[3], float* pdf, float* eta_out) {
    if (!params || params[0] != (float)kBsdfDielectric || !spec_trans || !wi || !wo || !value || !pdf || !eta_out)
        return fail(SDMM_E_INVALID, "sdmm_bsdf_roughdielectric_host: invalid argument (params of a kind-4 BSDF)");
    const unsigned csr = _mm_getcsr();
    _mm_setcsr(csr | 0x8040u);
    if (u) {
        float o[3];
        roughdielectric_sample(wi, params, spec_trans, u[0], u[1], u[2], o, value, pdf, eta_out);
        for (int a = 0; a < 3; ++a) wo[a] = o[a];
    } else {
        *pdf = roughdielectric_eval_pdf(wi, wo, params, spec_trans, value);
        *eta_out = roughdielectric_crossed_eta(wi, wo, params);
    }
    _mm_setcsr(csr);
    return SDMM_OK;
}

int sdmm_bsdf_roughdielectric_device(const float* params, const float spec_trans[3], int64_t nq,
                                     const float* const wi[3], const float* const* u, float* const wo[3],
                                     float* const value[3], float* pdf, float* eta_out, void* hip_stream) {
    if (!params || params[0] != (float)kBsdfDielectric || !spec_trans || nq < 0)
        return fail(SDMM_E_INVALID, "sdmm_bsdf_roughdielectric_device: invalid argument (params of a kind-4 BSDF)");
    if (nq == 0) return SDMM_OK;
    if (!wi || !wi[0] || !wi[1] || !wi[2] || !wo || !wo[0] || !wo[1] || !wo[2] || !value || !value[0] ||
        !value[1] || !value[2] || !pdf || !eta_out || (u && (!u[0] || !u[1] || !u[2])))
        return fail(SDMM_E_INVALID, "sdmm_bsdf_roughdielectric_device: NULL plane");
    HIP_TRY(launch_roughdielectric(params, spec_trans, nq, wi, u, wo, value, pdf, eta_out, (hipStream_t)hip_stream));
    return SDMM_OK;
}

int sdmm_bsdf_smooth_host(const float* params, const float spec_trans[3], const float wi[3], const float* u,
                          float wo[3], float value[3], float* pdf, float* eta_out) {
    if (!params || !is_smooth_kind(params[0]) || (params[0] == (float)kBsdfSmoothDielectric && !spec_trans) || !wi ||
        !wo || !value || !pdf || !eta_out)
        return fail(SDMM_E_INVALID, "sdmm_bsdf_smooth_host: invalid argument (params of a kind-5 or kind-6 BSDF)");
    const float none[3] = {0.0f, 0.0f, 0.0f};
    const float* st = spec_trans ? spec_trans : none;
    const unsigned csr = _mm_getcsr();
    _mm_setcsr(csr | 0x8040u);
    if (u) {
        float o[3];
        smooth_sample(wi, params, st, u[0], o, value, pdf, eta_out);
        for (int a = 0; a < 3; ++a) wo[a] = o[a];
    } else {
        *pdf = smooth_eval_pdf(wi, wo, params, st, value, eta_out);
    }
    _mm_setcsr(csr);
    return SDMM_OK;
}

int sdmm_bsdf_smooth_device(const float* params, const float spec_trans[3], int64_t nq, const float* const wi[3],
                            const float* const* u, float* const wo[3], float* const value[3], float* pdf,
                            float* eta_out, void* hip_stream) {
    if (!params || !is_smooth_kind(params[0]) || (params[0] == (float)kBsdfSmoothDielectric && !spec_trans) || nq < 0)
        return fail(SDMM_E_INVALID, "sdmm_bsdf_smooth_device: invalid argument (params of a kind-5 or kind-6 BSDF)");
    if (nq == 0) return SDMM_OK;
    if (!wi || !wi[0] || !wi[1] || !wi[2] || !wo || !wo[0] || !wo[1] || !wo[2] || !value || !value[0] ||
        !value[1] || !value[2] || !pdf || !eta_out || (u && (!u[0] || !u[1])))
        return fail(SDMM_E_INVALID, "sdmm_bsdf_smooth_device: NULL plane");
    HIP_TRY(launch_smooth(params, spec_trans, nq, wi, u, wo, value, pdf, eta_out, (hipStream_t)hip_stream));
    return SDMM_OK;
}

void sdmm_scene_destroy(sdmm_scene* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    (void)hipDeviceSynchronize();
    if (s->dquads) (void)hipFree(s->dquads);
    if (s->drefl) (void)hipFree(s->drefl);
    if (s->dbpar) (void)hipFree(s->dbpar);
    if (s->dlmod) (void)hipFree(s->dlmod);
    if (s->dlmod_nd) (void)hipFree(s->dlmod_nd);
    if (s->dtwosided) (void)hipFree(s->dtwosided);
    if (s->drad) (void)hipFree(s->drad);
    if (s->dnodes) (void)hipFree(s->dnodes);
    if (s->dtris) (void)hipFree(s->dtris);
    if (s->dhits) (void)hipFree(s->dhits);
    if (s->dshade) (void)hipFree(s->dshade);
    if (s->denv) (void)hipFree(s->denv);
    if (s->buf) (void)hipFree(s->buf);
    if (s->lt) (void)hipFree(s->lt);
    if (s->hcount) (void)hipHostFree(s->hcount);
    if (s->hfb) (void)hipHostFree(s->hfb);
    delete s;
}

int sdmm_scene_normalization(const sdmm_scene* s, float scene_min[3], float* spatial_norm, float tree_min[3],
                             float tree_max[3]) {
    if (!s) return fail(SDMM_E_INVALID, "null scene");
    for (int a = 0; a < 3; ++a) {
        if (scene_min) scene_min[a] = s->smin[a];
        if (tree_min) tree_min[a] = s->tmin[a];
        if (tree_max) tree_max[a] = s->tmax[a];
    }
    if (spatial_norm) *spatial_norm = s->snorm;
    return SDMM_OK;
}

int sdmm_scene_intersect(const sdmm_scene* s, int64_t nq, const float* const o[3], const float* const d[3], float mint,
                         float maxt, int mode, int32_t* prim, float* t, void* hip_stream) {
    if (!s || nq < 0 || (mode != 0 && mode != 1))
        return fail(SDMM_E_INVALID, "sdmm_scene_intersect: invalid argument (mode 0 or 1)");
    if (nq == 0) return SDMM_OK;
    if (!o || !o[0] || !o[1] || !o[2] || !d || !d[0] || !d[1] || !d[2] || !prim || !t)
        return fail(SDMM_E_INVALID, "sdmm_scene_intersect: NULL plane");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(launch_scene_intersect(s->S, nq, o, d, mint, maxt, mode, prim, t, (hipStream_t)hip_stream));
    return SDMM_OK;
}

int sdmm_scene_intersect_host(const sdmm_scene_desc* desc, int64_t nq, const float* o, const float* d, float mint,
                              float maxt, int mode, int32_t* prim, float* t) {
    return sdmm_scene_intersect_host_levels(desc, 0, nq, o, d, mint, maxt, mode, prim, t);
}

int sdmm_scene_intersect_host_levels(const sdmm_scene_desc* desc, int max_levels, int64_t nq, const float* o,
                                     const float* d, float mint, float maxt, int mode, int32_t* prim, float* t) {
    if (!desc || max_levels < 0 || nq < 0 || (mode != 0 && mode != 1) || (nq > 0 && (!o || !d || !prim || !t)))
        return fail(SDMM_E_INVALID, "sdmm_scene_intersect_host: invalid argument (mode 0 or 1)");
    std::vector<QuadDev> qs;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    int rc = prep_quads(desc, "sdmm_scene_intersect_host", &qs, mn, mx);
    if (rc) return rc;
    MeshBvh mesh;
    if (desc->n_triangles > 0) {
        rc = prep_mesh(desc, "sdmm_scene_intersect_host", max_levels, &mesh);
        if (rc) return rc;
    }
    // the device's float environment: denormals flushed (-fgpu-flush-denormals-to-zero)
    const unsigned csr = _mm_getcsr();
    _mm_setcsr(csr | 0x8040u);
    const int nquads = (int)qs.size();
    for (int64_t i = 0; i < nq; ++i) {
        float tb;
        int best = quads_closest(qs.data(), nquads, o + 3 * i, d + 3 * i, mint, maxt, tb);
        if (desc->n_triangles > 0) mesh_closest_host(mesh, nquads, mode, o + 3 * i, d + 3 * i, mint, maxt, best, tb);
        prim[i] = best;
        t[i] = tb;
    }
    _mm_setcsr(csr);
    return SDMM_OK;
}

int sdmm_scene_shading(const sdmm_scene* s, int64_t nq, const float* const o[3], const float* const d[3], float mint,
                       float maxt, int mode, int32_t* prim, float* t, float* const ns[3], float* const ng[3],
                       void* hip_stream) {
    if (!s || nq < 0 || (mode != 0 && mode != 1))
        return fail(SDMM_E_INVALID, "sdmm_scene_shading: invalid argument (mode 0 or 1)");
    if (nq == 0) return SDMM_OK;
    if (!o || !o[0] || !o[1] || !o[2] || !d || !d[0] || !d[1] || !d[2] || !prim || !t || !ns || !ns[0] || !ns[1] ||
        !ns[2] || !ng || !ng[0] || !ng[1] || !ng[2])
        return fail(SDMM_E_INVALID, "sdmm_scene_shading: NULL plane");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(launch_scene_shading(s->S, s->N.shade, nq, o, d, mint, maxt, mode, prim, t, ns, ng, (hipStream_t)hip_stream));
    return SDMM_OK;
}

int sdmm_scene_shading_host(const sdmm_scene_desc* desc, int64_t nq, const float* o, const float* d, float mint,
                            float maxt, int mode, int32_t* prim, float* t, float* ns, float* ng) {
    if (!desc || nq < 0 || (mode != 0 && mode != 1) || (nq > 0 && (!o || !d || !prim || !t || !ns || !ng)))
        return fail(SDMM_E_INVALID, "sdmm_scene_shading_host: invalid argument (mode 0 or 1)");
    std::vector<QuadDev> qs;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    int rc = prep_quads(desc, "sdmm_scene_shading_host", &qs, mn, mx);
    if (rc) return rc;
    MeshBvh mesh;
    if (desc->n_triangles > 0) {
        rc = prep_mesh(desc, "sdmm_scene_shading_host", 0, &mesh);
        if (rc) return rc;
    }
    // the scene as hit_normals reads it, on host arrays
    SceneDev S{};
    S.quads = qs.data();
    S.n_quads = (int)qs.size();
    S.hits = mesh.hits.data();
    const MeshShade* shade = mesh.shade.empty() ? nullptr : mesh.shade.data();
    // the device's float environment: denormals flushed (-fgpu-flush-denormals-to-zero)
    const unsigned csr = _mm_getcsr();
    _mm_setcsr(csr | 0x8040u);
    for (int64_t i = 0; i < nq; ++i) {
        float tb;
        int best = quads_closest(qs.data(), S.n_quads, o + 3 * i, d + 3 * i, mint, maxt, tb);
        if (desc->n_triangles > 0)
            mesh_closest_host(mesh, S.n_quads, mode, o + 3 * i, d + 3 * i, mint, maxt, best, tb);
        prim[i] = best;
        t[i] = tb;
        for (int a = 0; a < 3; ++a) ns[3 * i + a] = ng[3 * i + a] = 0.0f;
        if (best >= 0) hit_normals(S, shade, best, o + 3 * i, d + 3 * i, ns + 3 * i, ng + 3 * i);
    }
    _mm_setcsr(csr);
    return SDMM_OK;
}

int sdmm_env_eval(const sdmm_scene* s, int64_t nq, const float* const d[3], float* const rgb[3], void* hip_stream) {
    if (!s || nq < 0) return fail(SDMM_E_INVALID, "sdmm_env_eval: invalid argument");
    if (nq == 0) return SDMM_OK;
    if (!d || !d[0] || !d[1] || !d[2] || !rgb || !rgb[0] || !rgb[1] || !rgb[2])
        return fail(SDMM_E_INVALID, "sdmm_env_eval: NULL plane");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(launch_env_eval(s->S, nq, d, rgb, (hipStream_t)hip_stream));
    return SDMM_OK;
}

int sdmm_env_eval_host(const sdmm_scene_desc* desc, int64_t nq, const float* d, float* rgb) {
    if (!desc || nq < 0 || (nq > 0 && (!d || !rgb)))
        return fail(SDMM_E_INVALID, "sdmm_env_eval_host: invalid argument");
    EnvDev env;
    const int rc = prep_env(desc, "sdmm_env_eval_host", &env);
    if (rc) return rc;
    env.texels = desc->env_pixels;   // [h][w][3], read in place
    // the device's float environment: denormals flushed (-fgpu-flush-denormals-to-zero)
    const unsigned csr = _mm_getcsr();
    _mm_setcsr(csr | 0x8040u);
    for (int64_t i = 0; i < nq; ++i) env_eval<false>(env, d + 3 * i, rgb + 3 * i);
    _mm_setcsr(csr);
    return SDMM_OK;
}

int sdmm_mesh_bvh_dump(const sdmm_scene_desc* desc, int max_levels, int* n_nodes, int* levels, int cap_nodes,
                       float* boxes, int32_t* children, int32_t* order) {
    if (!desc || desc->n_triangles < 1 || max_levels < 0 || !n_nodes)
        return fail(SDMM_E_INVALID, "sdmm_mesh_bvh_dump: invalid argument (a description with triangles)");
    MeshBvh mesh;
    const int rc = prep_mesh(desc, "sdmm_mesh_bvh_dump", max_levels, &mesh);
    if (rc) return rc;
    *n_nodes = (int)mesh.nodes.size();
    if (levels) *levels = mesh.levels;
    if (cap_nodes <= 0) return SDMM_OK;
    if (cap_nodes < *n_nodes || !boxes || !children || !order)
        return fail(SDMM_E_INVALID, "sdmm_mesh_bvh_dump: arrays for fewer nodes than the tree has");
    for (size_t i = 0; i < mesh.nodes.size(); ++i) {
        const BvhNode& N = mesh.nodes[i];
        for (int c = 0; c < 2; ++c) {
            for (int a = 0; a < 3; ++a) {
                boxes[12 * i + 6 * c + a] = N.lo[c][a];
                boxes[12 * i + 6 * c + 3 + a] = N.hi[c][a];
            }
            children[2 * i + c] = N.child[c];
        }
    }
    for (size_t i = 0; i < mesh.tris.size(); ++i) order[i] = mesh.tris[i].id;
    return SDMM_OK;
}

int sdmm_li_render(sdmm_scene* s, sdmm_stree* t, const sdmm_mix* const* node_mix, const sdmm_li_params* p,
                   float* image, float* image_sqr, sdmm_path_vertices* vout, sdmm_li_stats* stats) {
    if (!s || !t || !p || !image) return fail(SDMM_E_INVALID, "invalid argument");
    const int64_t npix_all = (int64_t)s->S.width * s->S.height;
    if (p->spp < 1 || p->pixel_begin < 0 || p->pixel_end > npix_all || p->pixel_end <= p->pixel_begin ||
        p->rr_depth < 1 || p->max_depth == 0 || p->max_depth < -1 || p->saved_vertices < 1)
        return fail(SDMM_E_INVALID, "sdmm_li_render: invalid parameters");
    if (p->max_depth > 0 && p->saved_vertices < p->max_depth - 1)
        return fail(SDMM_E_INVALID, "sdmm_li_render: saved_vertices < max_depth - 1");
    if (p->guided && !(p->bsdf_fraction >= 0.0f && p->bsdf_fraction <= 1.0f))
        return fail(SDMM_E_INVALID, "sdmm_li_render: bsdf_fraction outside [0, 1]");
    const int product = p->sample_product ? 1 : 0;
    if (product) {
        const sdmm_bsdf_table& lb = p->learned_bsdf;
        if (lb.M < 1 || lb.M > 64 || lb.B < 1 || !lb.weights || !lb.means || !lb.covs)
            return fail(SDMM_E_INVALID, "sdmm_li_render: sample_product needs a learned-BSDF table (B >= 1, 1 <= M <= 64)");
    }
    const int64_t npix = p->pixel_end - p->pixel_begin;
    const int64_t P = npix * p->spp;
    if (P > INT32_MAX) return fail(SDMM_E_INVALID, "sdmm_li_render: at most 2^31 - 1 paths per call");
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = nullptr;
    int r = sdmm_detail::tree_stream(t, &st);
    if (r) return r;
    const int V = p->saved_vertices;
    r = grow(s, P, V, st);
    if (r) return r;
    s->P.V = V;
    s->P.P = P;
    s->N.strict = p->non_strict_normals ? 0 : 1;
    sdmm_bsdf_table ltab{};
    s->Q.lw = s->Q.lm = s->Q.lc = nullptr;
    if (product && p->guided && s->per_query_lobes) {
        r = extend_learned(s, p->learned_bsdf, s->cap_paths, st, &ltab);
        if (r) return r;
    }
    const int64_t path0 = p->pixel_begin * p->spp;
    HIP_TRY(launch_li_camera(s->S, s->P, s->N, path0, p->spp, p->seed, st));
    // bounces: rRec.depth 1 .. maxDepth - 1 scatter (:649, :684); unbounded
    // paths stop at the vertex slots
    const int bounces = p->max_depth > 0 ? p->max_depth - 1 : V;
    int64_t guided_queries = 0;
    if (!s->hcount) HIP_TRY(hipHostMalloc((void**)&s->hcount, sizeof(int32_t), hipHostMallocDefault));
    if (stats && p->guided && s->hfb_cap < bounces) {
        if (s->hfb) HIP_TRY(hipHostFree(s->hfb));
        s->hfb = nullptr;
        s->hfb_cap = 0;
        HIP_TRY(hipHostMalloc((void**)&s->hfb, sizeof(int32_t) * (size_t)bounces, hipHostMallocDefault));
        s->hfb_cap = bounces;
    }
    if (stats && p->guided)
        for (int b = 0; b < bounces; ++b) s->hfb[b] = 0;
    const float h = p->bsdf_fraction;
    for (int b = 0; b < bounces; ++b) {
        HIP_TRY(launch_li_query(s->S, s->P, s->Q, s->N, path0, b, p->max_depth > 0 ? p->max_depth : INT32_MAX, p->guided,
                                h, p->seed, st));
        if (p->guided) {
            // only the live paths query the guide: compact them (the order of
            // the compact queries does not change any query's outputs)
            HIP_TRY(launch_li_compact(s->S, s->P, s->Q, s->N, P, s->dcount, s->temp, s->temp_bytes, product, st));
            HIP_TRY(hipMemcpyAsync(s->hcount, s->dcount, sizeof(int32_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            const int64_t nlive = *s->hcount;
            const float* c[3] = {s->Q.k_c0, s->Q.k_c1, s->Q.k_c2};
            const float* u[3] = {s->Q.k_u0, s->Q.k_u1, s->Q.k_u2};
            const float* bd[3] = {s->Q.k_b0, s->Q.k_b1, s->Q.k_b2};
            float* d[3] = {s->Q.d0, s->Q.d1, s->Q.d2};
            if (nlive > 0) {
                if (product) {
                    // sampleSurface with sampleProduct (:327-392): the product
                    // of the leaf's conditional and the material's learned
                    // BSDF, h = 0.3 (0.5 without a usable product), the BSDF /
                    // guide choice taken against the query's own h
                    const float* F[9];
                    for (int i = 0; i < 9; ++i) F[i] = s->Q.k_F[i];
                    r = sdmm_guide_product_wavefront(t, node_mix, nlive, c, u, s->Q.k_ch, bd,
                                                     s->Q.lw ? &ltab : &p->learned_bsdf, s->Q.k_mat, F, d,
                                                     s->Q.pdf, s->Q.comp, s->Q.hq, nullptr);
                } else {
                    r = sdmm_guide_pdf_wavefront(t, node_mix, nlive, c, u, bd, s->Q.k_mode, d, s->Q.pdf,
                                                 s->Q.comp, nullptr);
                }
                if (r) return r;
                // (stream-ordered copy, read after the final synchronisation)
                const int* fb = sdmm_detail::tree_fallback_count(t);
                if (stats && fb)
                    HIP_TRY(hipMemcpyAsync(s->hfb + b, fb, sizeof(int32_t), hipMemcpyDeviceToHost, st));
            }
            guided_queries += nlive;
        }
        HIP_TRY(launch_li_shade(s->S, s->P, s->Q, s->N, path0, b, p->rr_depth, h, p->seed, product && p->guided, st));
    }
    HIP_TRY(launch_li_film(s->P, p->pixel_begin, npix, p->spp, npix_all, image, image_sqr, st));
    if (vout) {
        vout->n_paths = P;
        vout->max_vertices = V;
        vout->path0 = path0;
        vout->rec = s->P.rec;
        vout->nv = s->P.nv;
    }
    if (stats) {
        // traced bounce rays (a delta lobe's ray saves no vertex)
        size_t tb = s->temp_bytes;
        HIP_TRY(hipcub::DeviceReduce::Sum(s->temp, tb, (const int32_t*)s->P.nray, s->dsum, (int)P, st));
        int64_t seg = 0;
        HIP_TRY(hipMemcpyAsync(&seg, s->dsum, sizeof(int64_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        stats->paths = P;
        stats->segments = seg;
        stats->guided_queries = guided_queries;
        stats->fallback_queries = 0;
        if (p->guided)
            for (int b = 0; b < bounces; ++b) stats->fallback_queries += s->hfb[b];
    }
    return SDMM_OK;
}

}  // extern "C"
