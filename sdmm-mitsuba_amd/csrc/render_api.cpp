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
#include <type_traits>
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
    std::vector<void*> owned;   // the device blocks behind S, N.shade, T and S.env.texels (upload), freed by destroy
    float smin[3] = {0, 0, 0}, snorm = 1.0f, tmin[3] = {0, 0, 0}, tmax[3] = {0, 0, 0};
    // per-render buffers (grown)
    void* buf = nullptr;
    size_t buf_bytes = 0;
    int64_t cap_paths = 0;
    int cap_v = 0;
    PathsDev P{};
    QueryDev Q{};
    NormalsDev N{};   // (vertex normals: N.shade the scene's, the ns / ng planes in buf)
    TexDev T{};       // (textures: T.tex, bsdf_tex, mesh_uv the scene's, the reflectance planes in buf)
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

constexpr size_t align256(size_t bytes) { return (bytes + 255) / 256 * 256; }

// The per-render arena of `cap` paths with `cv` vertex slots and `tb` bytes of
// hipcub scratch: the path, query and vertex planes one after the other, each
// on a 256-byte boundary.  base set: s->P, Q, N, T, dsum, temp and dcount point
// into it; null: nothing is assigned.  Returns the arena's bytes either way.
size_t layout_paths(sdmm_scene* s, char* base, int64_t cap, int cv, size_t tb) {
    size_t off = 0;
    auto take = [&](auto*& p, size_t bytes) {
        if (base) p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(base + off);
        off += align256(bytes);
    };
    const size_t f = sizeof(float) * (size_t)cap, i4 = sizeof(int32_t) * (size_t)cap, u1 = (size_t)cap;
    PathsDev& P = s->P;
    QueryDev& Q = s->Q;
    NormalsDev& N = s->N;
    for (float** p : {&P.px, &P.py, &P.pz, &P.dx, &P.dy, &P.dz, &P.tr, &P.tg, &P.tb, &P.lr, &P.lg, &P.lb}) take(*p, f);
    take(P.depth, i4);
    take(P.quad, i4);
    take(P.nv, i4);
    take(P.nray, i4);
    take(P.rec, sizeof(float) * (size_t)kVertexFields * (size_t)cv * (size_t)cap);
    for (float** p : {&Q.c0, &Q.c1, &Q.c2, &Q.u0, &Q.u1, &Q.u2, &Q.b0, &Q.b1, &Q.b2, &Q.d0, &Q.d1, &Q.d2, &Q.pdf})
        take(*p, f);
    take(Q.mode, u1);
    take(Q.comp, i4);
    take(s->dsum, sizeof(int64_t));
    take(s->temp, tb);
    if (base) s->temp_bytes = align256(tb);
    for (float** p : {&Q.k_c0, &Q.k_c1, &Q.k_c2, &Q.k_u0, &Q.k_u1, &Q.k_u2, &Q.k_b0, &Q.k_b1, &Q.k_b2}) take(*p, f);
    take(Q.k_mode, u1);
    take(Q.live, u1);
    take(Q.idx, i4);
    take(Q.slot, i4);
    take(s->dcount, i4);
    take(Q.ch, f);
    take(Q.k_ch, f);
    for (float*& p : Q.k_F) take(p, f);
    take(Q.hq, f);
    take(Q.k_mat, i4);
    take(Q.bdelta, u1);
    for (float** p : {&Q.bw0, &Q.bw1, &Q.bw2, &Q.bpdf}) take(*p, f);
    // the eta planes: only with a dielectric or a kind-5 / 6 BSDF; the ns / ng
    // planes: only with vertex normals; the reflectance planes: only with a
    // textured BSDF (null otherwise, as created)
    if (s->S.has_dielectric) {
        take(P.eta, f);
        take(Q.beta, f);
    }
    if (N.shade)
        for (float** p : {&N.nsx, &N.nsy, &N.nsz, &N.ngx, &N.ngy, &N.ngz}) take(*p, f);
    if (s->T.bsdf_tex)
        for (float** p : {&s->T.rr, &s->T.rg, &s->T.rb}) take(*p, f);
    return off;
}

// path + query + vertex planes for P paths with V vertex slots
int grow(sdmm_scene* s, int64_t P, int V, hipStream_t st) {
    if (P <= s->cap_paths && V <= s->cap_v && s->buf) return SDMM_OK;
    const int64_t cap = std::max<int64_t>(P, s->cap_paths);
    const int cv = std::max(V, s->cap_v);
    size_t tb = 0;
    (void)hipcub::DeviceReduce::Sum(nullptr, tb, (const int32_t*)nullptr, (int64_t*)nullptr, (int)cap);
    tb = std::max(tb, li_select_temp_bytes(cap));
    const size_t need = layout_paths(s, nullptr, cap, cv, tb);
    HIP_TRY(hipStreamSynchronize(st));
    if (s->buf) HIP_TRY(hipFree(s->buf));
    s->buf = nullptr;
    HIP_TRY(hipMalloc(&s->buf, need));
    s->buf_bytes = need;
    s->cap_paths = cap;
    s->cap_v = cv;
    layout_paths(s, (char*)s->buf, cap, cv, tb);
    return SDMM_OK;
}

// the four blocks of an extended learned-BSDF table of `rows` rows of lM
// lobes (weights, means, covariances, diffuse flags), laid out like the arena
struct LearnedBlocks {
    float *w, *m, *c;
    uint8_t* dflag;
};
size_t layout_learned(LearnedBlocks* L, char* base, int64_t rows, int lM) {
    size_t off = 0;
    auto take = [&](auto*& p, size_t bytes) {
        if (base) p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(base + off);
        off += bytes;
    };
    const size_t wb = align256(sizeof(float) * (size_t)rows * lM);
    take(L->w, wb);
    take(L->m, 3 * wb);
    take(L->c, 4 * wb);
    take(L->dflag, align256((size_t)rows));
    return off;
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
    LearnedBlocks L{};
    const size_t need = layout_learned(&L, nullptr, rows, lM);
    if (need > s->lt_bytes) {
        HIP_TRY(hipStreamSynchronize(st));
        if (s->lt) HIP_TRY(hipFree(s->lt));
        s->lt = nullptr;
        s->lt_bytes = 0;
        HIP_TRY(hipMalloc(&s->lt, need));
        s->lt_bytes = need;
    }
    layout_learned(&L, (char*)s->lt, rows, lM);
    HIP_TRY(hipMemsetAsync(L.w, 0, sizeof(float) * (size_t)B * lM, st));
    HIP_TRY(hipMemcpy2DAsync(L.w, sizeof(float) * lM, user.weights, sizeof(float) * M, sizeof(float) * M, B,
                             hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemsetAsync(L.m, 0, sizeof(float) * 3 * (size_t)B * lM, st));
    HIP_TRY(hipMemcpy2DAsync(L.m, sizeof(float) * 3 * lM, user.means, sizeof(float) * 3 * M, sizeof(float) * 3 * M, B,
                             hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemsetAsync(L.c, 0, sizeof(float) * 4 * (size_t)B * lM, st));
    HIP_TRY(hipMemcpy2DAsync(L.c, sizeof(float) * 4 * lM, user.covs, sizeof(float) * 4 * M, sizeof(float) * 4 * M, B,
                             hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemsetAsync(L.dflag, 0, (size_t)rows, st));
    if (user.diffuse) HIP_TRY(hipMemcpyAsync(L.dflag, user.diffuse, (size_t)B, hipMemcpyDeviceToDevice, st));
    *tab = sdmm_bsdf_table{L.w, L.m, L.c, (int)std::min<int64_t>(rows, INT32_MAX), lM, L.dflag};
    s->Q.lw = L.w;
    s->Q.lm = L.m;
    s->Q.lc = L.c;
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
int check_emitters(const sdmm_scene_desc* d, const char* who) {
    if (has_emitters(d) && (d->n_emitters < 1 || !d->radiance))
        return fail(SDMM_E_INVALID, std::string(who) + ": emitters without radiance");
    return SDMM_OK;
}

// BSDF b's kind (render_device.h); without bsdf_params every BSDF is diffuse
float bsdf_kind(const sdmm_scene_desc* d, int b) {
    return d->bsdf_params ? d->bsdf_params[kBsdfParams * b] : (float)kBsdfDiffuse;
}
// a color triple: no negative channel, a finite sum
bool rgb_ok(const float* c) {
    return c[0] >= 0.0f && c[1] >= 0.0f && c[2] >= 0.0f && std::isfinite(c[0] + c[1] + c[2]);
}
// a bsdf_params row's specular reflectance (slots 1 .. 3)
bool spec_ok(const float* bp) { return rgb_ok(bp + 1); }
// one BSDF's bsdf_params row (render_device.h): its kind one of 0 .. 6, that
// kind's slots in range (the plastic kind tests no finiteness)
bool bsdf_params_ok(const float* bp) {
    const auto fin = [](float x) { return std::isfinite(x); };
    // eta = intIOR / extIOR of a dielectric and its inverse
    const auto eta_ok = [&] { return bp[4] > 0.0f && bp[4] != 1.0f && fin(bp[4]) && bp[5] > 0.0f && fin(bp[5]); };
    // a conductor's gray eta and k
    const auto eta_k_ok = [&] { return bp[4] > 0.0f && fin(bp[4]) && bp[5] >= 0.0f && fin(bp[5]); };
    const auto alpha_ok = [&] { return bp[6] > 0.0f && bp[6] <= 2.0f; };
    int kind = -1;
    for (int k = kBsdfDiffuse; k <= kBsdfSmoothConductor; ++k)
        if (bp[0] == (float)k) kind = k;
    switch (kind) {
        case kBsdfDiffuse: return true;
        case kBsdfPlastic: return bp[4] > 0.0f && bp[5] > 0.0f && bp[6] < 1.0f && bp[7] >= 0.0f && bp[7] <= 1.0f;
        case kBsdfConductor: return spec_ok(bp) && eta_k_ok() && alpha_ok();
        case kBsdfPhong: return spec_ok(bp) && bp[4] >= 0.0f && fin(bp[4]) && bp[5] >= 0.0f && bp[5] <= 1.0f;
        case kBsdfDielectric: return spec_ok(bp) && eta_ok() && alpha_ok();
        case kBsdfSmoothDielectric: return spec_ok(bp) && eta_ok();
        case kBsdfSmoothConductor: return spec_ok(bp) && eta_k_ok();
        default: return false;
    }
}
// the kinds that condition a learned model per bounce (per-query lobes)
bool per_query_kind(float kind) {
    return kind == (float)kBsdfConductor || kind == (float)kBsdfPhong || kind == (float)kBsdfDielectric;
}

// the model's records (kLearnedRec / learned_rec(C) floats each) from the ABI
// arrays; false: not a model (C, M or a missing array)
bool pack_records(int C, int M, const float* weights, const float* means, const float* covs, float* rec) {
    if ((C != 2 && C != 3) || M < 0 || M > kLearnedMaxComp || (M > 0 && (!weights || !means || !covs))) return false;
    const int R = learned_rec(C), nm = C + 3, nc = (C + 2) * (C + 2);
    for (int k = 0; k < M; ++k) {
        float* r = rec + R * k;
        r[0] = weights[k];
        for (int i = 0; i < nm; ++i) r[1 + i] = means[nm * k + i];
        for (int i = 0; i < nc; ++i) r[1 + nm + i] = covs[nc * k + i];
    }
    return true;
}
static_assert(learned_rec(2) == kLearnedRec, "an SDMM4 record is the C = 2 record");
bool pack_learned4(const sdmm_learned_bsdf4* m, float* rec) {
    return m && pack_records(2, m->M, m->weights, m->means, m->covs, rec);
}
bool pack_learned(const sdmm_learned_bsdf* m, float* rec) {
    return m && pack_records(m->C, m->M, m->weights, m->means, m->covs, rec);
}
// M packed records over a C-dimensional condition: every value finite, no
// negative weight, the mean's direction (after the condition) a unit vector
bool learned_records_ok(const float* rec, int C, int M) {
    const int R = learned_rec(C);
    for (int k = 0; k < M; ++k) {
        const float *r = rec + R * k, *dir = r + 1 + C;
        bool ok = r[0] >= 0.0f;
        for (int i = 0; i < R; ++i) ok = ok && std::isfinite(r[i]);
        const double n2 = (double)dir[0] * dir[0] + (double)dir[1] * dir[1] + (double)dir[2] * dir[2];
        if (!ok || std::fabs(n2 - 1.0) > 1e-5) return false;
    }
    return true;
}

// the device's float environment on this thread while in scope: denormals
// flushed (-fgpu-flush-denormals-to-zero)
struct DeviceFloatEnv {
    const unsigned csr = _mm_getcsr();
    DeviceFloatEnv() { _mm_setcsr(csr | 0x8040u); }
    ~DeviceFloatEnv() { _mm_setcsr(csr); }
    DeviceFloatEnv(const DeviceFloatEnv&) = delete;
    DeviceFloatEnv& operator=(const DeviceFloatEnv&) = delete;
};

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

// the description's two-sided flags, validated (after geometry_args_ok); *any:
// some entry is set.  0, or the error code (message set).
int prep_twosided(const sdmm_scene_desc* d, const char* who, bool* any) {
    const std::string w(who);
    *any = false;
    if (!d->bsdf_twosided) return SDMM_OK;
    for (int b = 0; b < d->n_bsdfs; ++b) {
        const int32_t v = d->bsdf_twosided[b];
        if (v != 0 && v != 1) return fail(SDMM_E_INVALID, w + ": a bsdf_twosided entry other than 0 or 1");
        if (v == 0) continue;
        // "Only materials without a transmission component can be nested" (twosided.cpp:106-108)
        const float kind = bsdf_kind(d, b);
        if (kind == (float)kBsdfDielectric || kind == (float)kBsdfSmoothDielectric)
            return fail(SDMM_E_INVALID, w + ": bsdf_twosided on a transmitting BSDF (kind 4 or 5)");
        *any = true;
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

// A description's geometry on the host, as sdmm_scene_create uploads it and
// the *_host entries read it: the quads' derived data (normal, duals), the
// mesh with its BVH (has_mesh), the AABB of the quads' corners and the mesh's
// vertices (without the camera), and whether some BSDF is two-sided.
struct HostScene {
    std::vector<QuadDev> quads;
    MeshBvh mesh;
    bool has_mesh = false, twosided = false;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
};

// validates the description's geometry and material arguments and builds
// *hs.  0, or the error code (message set).
int build_host_scene(const sdmm_scene_desc* d, const char* who, int max_levels, HostScene* hs) {
    const std::string w(who);
    if (!geometry_args_ok(d)) return fail(SDMM_E_INVALID, w + ": invalid description");
    if (d->mesh_normals && d->n_triangles < 1) return fail(SDMM_E_INVALID, w + ": mesh_normals without triangles");
    if (const int rc = prep_twosided(d, who, &hs->twosided)) return rc;
    if (const int rc = check_emitters(d, who)) return rc;
    hs->quads.assign((size_t)d->n_quads, QuadDev{});
    for (int q = 0; q < d->n_quads; ++q) {
        QuadDev& Q = hs->quads[(size_t)q];
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
        for (int c = 0; c < 4; ++c)
            for (int a = 0; a < 3; ++a) {
                const float x = Q.p0[a] + ((c & 1) ? Q.e1[a] : 0.0f) + ((c & 2) ? Q.e2[a] : 0.0f);
                hs->mn[a] = std::min(hs->mn[a], x);
                hs->mx[a] = std::max(hs->mx[a], x);
            }
    }
    hs->has_mesh = d->n_triangles > 0;
    if (hs->has_mesh) {
        if (const int rc = prep_mesh(d, who, max_levels, &hs->mesh)) return rc;
        for (int a = 0; a < 3; ++a) {
            hs->mn[a] = std::min(hs->mn[a], hs->mesh.mn[a]);
            hs->mx[a] = std::max(hs->mx[a], hs->mesh.mx[a]);
        }
    }
    return SDMM_OK;
}

// The description's texture fields, validated (after every other check of the
// description, the geometry's included): the textures as texture.h reads them
// (texels: the caller's [h][w][3] arrays, in place), the per-triangle uv table
// (with triangles and either mesh_uvs or a texture), and whether some BSDF
// carries a texture.  0, or the error code (message set).
struct HostTextures {
    std::vector<TextureDev> tex;
    std::vector<MeshUV> mesh_uv;
    bool textured = false;
};
int prep_textures(const sdmm_scene_desc* d, const char* who, const HostScene& hs, HostTextures* ht) {
    const std::string w(who);
    if (d->mesh_uvs) {
        if (d->n_triangles < 1) return fail(SDMM_E_INVALID, w + ": mesh_uvs without triangles");
        for (int64_t i = 0; i < 2 * (int64_t)d->n_mesh_vertices; ++i)
            if (!std::isfinite(d->mesh_uvs[i])) return fail(SDMM_E_INVALID, w + ": a non-finite mesh_uvs value");
    }
    if (d->n_textures < 0 || (d->n_textures > 0 && !d->textures))
        return fail(SDMM_E_INVALID, w + ": n_textures < 0, or textures NULL with n_textures > 0");
    if (d->bsdf_texture && d->n_textures < 1) return fail(SDMM_E_INVALID, w + ": bsdf_texture without textures");
    int64_t total = 0;
    for (int i = 0; i < d->n_textures; ++i) {
        const sdmm_texture& t = d->textures[i];
        if (t.width < 1 || t.height < 1) return fail(SDMM_E_INVALID, w + ": a texture's width or height < 1");
        if (!t.pixels) return fail(SDMM_E_INVALID, w + ": a texture without pixels");
        total += (int64_t)t.width * t.height;
        if (total > kTexMaxTexels) return fail(SDMM_E_INVALID, w + ": textures of more than 2^26 texels in all");
        if (t.filter != kTexBilinear && t.filter != kTexNearest)
            return fail(SDMM_E_INVALID, w + ": a texture's filter outside 0..1");
        if (t.wrap_u < kWrapRepeat || t.wrap_u > kWrapOne || t.wrap_v < kWrapRepeat || t.wrap_v > kWrapOne)
            return fail(SDMM_E_INVALID, w + ": a texture's wrap_u or wrap_v outside 0..4");
        for (int a = 0; a < 2; ++a) {
            if (t.uv_scale[a] == 0.0f || !std::isfinite(t.uv_scale[a]))
                return fail(SDMM_E_INVALID, w + ": a texture's uv_scale is 0 or not finite");
            if (!std::isfinite(t.uv_offset[a])) return fail(SDMM_E_INVALID, w + ": a texture's uv_offset is not finite");
        }
        for (int64_t k = 0; k < 3 * (int64_t)t.width * t.height; ++k)
            if (!(std::isfinite(t.pixels[k]) && t.pixels[k] >= 0.0f))
                return fail(SDMM_E_INVALID, w + ": a non-finite or negative texel");
        ht->tex.push_back(TextureDev{t.pixels, t.width, t.height, t.filter, t.wrap_u, t.wrap_v,
                                     {t.uv_scale[0], t.uv_scale[1]}, {t.uv_offset[0], t.uv_offset[1]}});
    }
    if (d->bsdf_texture)
        for (int b = 0; b < d->n_bsdfs; ++b) {
            const int32_t ti = d->bsdf_texture[b];
            if (ti < -1 || ti >= d->n_textures)
                return fail(SDMM_E_INVALID, w + ": a bsdf_texture entry outside -1 .. n_textures - 1");
            if (ti < 0) continue;
            const float kind = bsdf_kind(d, b);
            if (kind != (float)kBsdfDiffuse && kind != (float)kBsdfPlastic && kind != (float)kBsdfPhong)
                return fail(SDMM_E_INVALID, w + ": bsdf_texture on a BSDF of kind 2, 4, 5 or 6 (only the reflectance "
                                                "of kinds 0, 1 and 3 takes a texture)");
            ht->textured = true;
        }
    if (hs.has_mesh && (d->mesh_uvs || d->n_textures > 0)) {
        ht->mesh_uv.assign((size_t)d->n_triangles, MeshUV{});
        for (const MeshTri& T : hs.mesh.tris) {
            MeshUV& V = ht->mesh_uv[(size_t)T.id];
            V.tri = T;
            if (!d->mesh_uvs) continue;
            const int32_t* ix = d->triangles + 3 * (int64_t)T.id;
            for (int a = 0; a < 2; ++a) {
                V.t0[a] = d->mesh_uvs[2 * (int64_t)ix[0] + a];
                V.t1[a] = d->mesh_uvs[2 * (int64_t)ix[1] + a];
                V.t2[a] = d->mesh_uvs[2 * (int64_t)ix[2] + a];
            }
            V.has_uv = 1;
        }
    }
    return SDMM_OK;
}

// the closest hit of the ray (o, d) with t in (mint, maxt) among the quads and
// the triangles (mode 0: the BVH, 1: the loop over all of them): the
// primitive or -1, *t its distance (maxt without one)
int closest(const HostScene& hs, int mode, const float o[3], const float d[3], float mint, float maxt, float* t) {
    const int nquads = (int)hs.quads.size();
    int best = quads_closest(hs.quads.data(), nquads, o, d, mint, maxt, *t);
    if (hs.has_mesh) mesh_closest_host(hs.mesh, nquads, mode, o, d, mint, maxt, best, *t);
    return best;
}

// n elements of host memory as a device block of max(n, alloc) elements that
// sdmm_scene_destroy frees; *out: the block.  Nothing to hold: *out stays.
template <class T>
hipError_t upload(sdmm_scene* s, const T* host, size_t n, const T** out, size_t alloc = 0) {
    alloc = std::max(n, alloc);
    if (alloc == 0) return hipSuccess;
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, sizeof(T) * alloc);
    if (e != hipSuccess) return e;
    s->owned.push_back(p);
    *out = static_cast<const T*>(p);
    return n ? hipMemcpy(p, host, sizeof(T) * n, hipMemcpyHostToDevice) : hipSuccess;
}

}  // namespace

extern "C" {

int sdmm_scene_create(const sdmm_scene_desc* d, int device, sdmm_scene** out) {
    const char* who = "sdmm_scene_create";
    const std::string w(who);
    if (!out || !d || !geometry_args_ok(d) || d->width < 1 || d->height < 1 ||
        !(d->fov_x_deg > 0.0f && d->fov_x_deg < 180.0f))
        return fail(SDMM_E_INVALID, w + ": invalid description");
    if (const int rc = check_emitters(d, who)) return rc;
    if (d->bsdf_params)
        for (int b = 0; b < d->n_bsdfs; ++b) {
            if (!bsdf_params_ok(d->bsdf_params + kBsdfParams * b))
                return fail(SDMM_E_INVALID, w + ": invalid bsdf_params");
            // a smooth dielectric's specularTransmittance (its reflectance row)
            if (bsdf_kind(d, b) == (float)kBsdfSmoothDielectric && !rgb_ok(d->reflectance + 3 * b))
                return fail(SDMM_E_INVALID, w + ": invalid bsdf_params (a smooth dielectric's transmittance is "
                                                "negative or not finite)");
        }
    // learned models: at most kLearnedMaxComp components, finite, unit
    // directions.  M == 0: none; a delta-only BSDF never calls getDMM: its
    // entry is not read, not even checked
    const auto no_model = [&](int b, int M) { return M == 0 || is_smooth_kind(bsdf_kind(d, b)); };
    const std::string bad_records =
        w + ": learned model with a non-finite value, a negative weight or a non-unit direction";
    std::vector<float> lmod;
    if (d->learned_models) {
        lmod.assign((size_t)kLearnedStride * (size_t)d->n_bsdfs, 0.0f);
        for (int b = 0; b < d->n_bsdfs; ++b) {
            const sdmm_learned_bsdf4& L = d->learned_models[b];
            if (no_model(b, L.M)) continue;
            float* o = lmod.data() + (size_t)kLearnedStride * b;
            if (!pack_learned4(&L, o + 1))
                return fail(SDMM_E_INVALID, w + ": invalid learned model (1 <= M <= 8, arrays)");
            o[0] = (float)L.M;
            if (!learned_records_ok(o + 1, 2, L.M)) return fail(SDMM_E_INVALID, bad_records);
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
            if (no_model(b, L.M)) continue;
            float* o = lmod_nd.data() + (size_t)kLearnedNdStride * b;
            if (!pack_learned(&L, o + 2))
                return fail(SDMM_E_INVALID, w + ": invalid learned model (C 2 or 3, 1 <= M <= 8, arrays)");
            if (bsdf_kind(d, b) == (float)kBsdfPhong && (L.C != 3 || L.M <= kPhongDiffuseComponent))
                return fail(SDMM_E_INVALID, w + ": a Phong BSDF's learned model needs C = 3 and M >= 2");
            if (bsdf_kind(d, b) == (float)kBsdfDielectric && L.C != 3)
                return fail(SDMM_E_INVALID, w + ": a rough dielectric's learned model needs C = 3");
            o[0] = (float)L.C;
            o[1] = (float)L.M;
            if (!learned_records_ok(o + 2, L.C, L.M)) return fail(SDMM_E_INVALID, bad_records);
        }
    }
    *out = nullptr;
    // the quads' derived data, the triangle mesh with its BVH, their AABB
    HostScene hs;
    int rc = build_host_scene(d, who, 0, &hs);
    if (rc) return rc;
    // the environment emitter: validated, a lat-long map as RGBA texels (envmap.h)
    EnvDev env;
    rc = prep_env(d, who, &env);
    if (rc) return rc;
    std::vector<EnvTexel> env_texels;
    if (env.kind == kEnvLatLong) {
        env_texels.resize((size_t)env.w * (size_t)env.h);
        for (size_t i = 0; i < env_texels.size(); ++i)
            env_texels[i] = EnvTexel{d->env_pixels[3 * i], d->env_pixels[3 * i + 1], d->env_pixels[3 * i + 2], 0.0f};
    }
    // the textures: validated (the last checks), as RGBA texels (texture.h)
    HostTextures ht;
    rc = prep_textures(d, who, hs, &ht);
    if (rc) return rc;
    std::vector<std::vector<TexTexel>> tex_texels(ht.tex.size());
    for (size_t i = 0; i < ht.tex.size(); ++i) {
        const float* px = ht.tex[i].texels;
        tex_texels[i].resize((size_t)ht.tex[i].w * (size_t)ht.tex[i].h);
        for (size_t k = 0; k < tex_texels[i].size(); ++k)
            tex_texels[i][k] = TexTexel{px[3 * k], px[3 * k + 1], px[3 * k + 2], 0.0f};
    }
    sdmm_scene* s = new (std::nothrow) sdmm_scene();
    if (!s) return fail(SDMM_E_NOMEM, "out of host memory");
    s->device = device;
    // (a conductor, Phong BSDF or rough dielectric some primitive uses: the CPU restatement's rule)
    for (int q = 0; q < d->n_quads; ++q)
        if (per_query_kind(bsdf_kind(d, d->bsdf[q]))) s->per_query_lobes = true;
    for (int i = 0; i < d->n_triangles; ++i)
        if (per_query_kind(bsdf_kind(d, d->tri_bsdf[i]))) s->per_query_lobes = true;
    // render() (volpath_sdmm.cpp:375-393): spatialNormalization = the largest
    // extent; the tree box getAABB (:314-332)
    float ext[3], norm = 0.0f;
    for (int a = 0; a < 3; ++a) { ext[a] = hs.mx[a] - hs.mn[a]; norm = std::max(norm, ext[a]); }
    for (int a = 0; a < 3; ++a) {
        s->smin[a] = hs.mn[a];
        s->tmin[a] = 0.0f - 1e-5f;
        s->tmax[a] = ext[a] / norm + 1e-5f;
    }
    s->snorm = norm;
    // the device tables: an empty one (no mesh, no vertex normals, no map, no
    // emitter, no bsdf_params, no model, no two-sided entry, no texture) stays null
    SceneDev& S = s->S;
    hipError_t e = hipSetDevice(device);
    const auto up = [&](const auto* host, size_t n, auto out, size_t alloc = 0) {
        if (e == hipSuccess) e = upload(s, host, n, out, alloc);
    };
    const size_t nb = (size_t)d->n_bsdfs;
    const EnvTexel* texels = nullptr;
    up(hs.quads.data(), hs.quads.size(), &S.quads, 1);
    up(hs.mesh.nodes.data(), hs.mesh.nodes.size(), &S.nodes);
    up(hs.mesh.tris.data(), hs.mesh.tris.size(), &S.tris);
    up(hs.mesh.hits.data(), hs.mesh.hits.size(), &S.hits);
    up(hs.mesh.shade.data(), hs.mesh.shade.size(), &s->N.shade);
    up(env_texels.data(), env_texels.size(), &texels);
    up(d->reflectance, 3 * nb, &S.refl);
    up(d->radiance, has_emitters(d) ? 3 * (size_t)d->n_emitters : 0, &S.rad);
    up(d->bsdf_params, d->bsdf_params ? kBsdfParams * nb : 0, &S.bpar);
    up(lmod.data(), lmod.size(), &S.lmodel);
    up(lmod_nd.data(), lmod_nd.size(), &S.lmodel_nd);
    up(d->bsdf_twosided, hs.twosided ? nb : 0, &S.twosided);
    for (size_t i = 0; i < ht.tex.size(); ++i) {
        const TexTexel* tx = nullptr;
        up(tex_texels[i].data(), tex_texels[i].size(), &tx);
        ht.tex[i].texels = reinterpret_cast<const float*>(tx);
    }
    up(ht.tex.data(), ht.tex.size(), &s->T.tex);
    up(d->bsdf_texture, ht.textured ? nb : 0, &s->T.bsdf_tex);
    up(ht.mesh_uv.data(), ht.mesh_uv.size(), &s->T.mesh_uv);
    if (e != hipSuccess) {
        sdmm_scene_destroy(s);
        return fail(SDMM_E_HIP, w + ": " + hipGetErrorString(e));
    }
    S.n_quads = d->n_quads;
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
    S.env = env;
    S.env.texels = reinterpret_cast<const float*>(texels);
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
    float rec[kLearnedMaxComp * kLearnedRec];
    if (!pack_learned4(m, rec) || !wi_local || !n_out || keep < 1 || !weights || !means || !covs)
        return fail(SDMM_E_INVALID, "sdmm_learned4_conditional: invalid argument");
    *n_out = 0;
    if (m->M == 0 || !(wi_local[2] > 0.0f)) return SDMM_OK;   // getDMM: no model, or cosTheta(wi) <= 0
    float w[kLearnedMaxComp], mm[3 * kLearnedMaxComp], cc[4 * kLearnedMaxComp];
    int n;
    {
        const DeviceFloatEnv env;
        const float theta = (float)std::acos((double)std::fmin(1.0f, wi_local[2]));
        n = learned4_conditional(rec, m->M, theta, alpha, wi_local, keep, w, mm, cc);
    }
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
    float rec[kLearnedMaxComp * kLearnedRec];
    if (!pack_learned4(m, rec) || nq < 0 || keep < 1 || keep > kLearnedMaxComp)
        return fail(SDMM_E_INVALID, "sdmm_learned4_conditional_device: invalid argument");
    if (nq == 0) return SDMM_OK;
    if (!wi_local || !wi_local[0] || !wi_local[1] || !wi_local[2] || !weights || !means || !covs || !n_out)
        return fail(SDMM_E_INVALID, "sdmm_learned4_conditional_device: invalid argument");
    HIP_TRY(launch_learned4(rec, m->M, alpha, nq, wi_local, keep, weights, means, covs, n_out,
                            (hipStream_t)hip_stream));
    return SDMM_OK;
}

int sdmm_learned_conditional(const sdmm_learned_bsdf* m, const float* cond_rest, const float wi_local[3], int keep,
                             int force, int* n_out, float* weights, float* means, float* covs) {
    float rec[kLearnedMaxComp * learned_rec(kLearnedMaxCond)];
    if (!pack_learned(m, rec) || !cond_rest || !wi_local || !n_out || keep < 0 || keep > kLearnedMaxComp ||
        force < -1 || force >= m->M || !weights || !means || !covs)
        return fail(SDMM_E_INVALID, "sdmm_learned_conditional: invalid argument (C 2 or 3, M <= 8, 0 <= keep <= 8, "
                                    "-1 <= force < M)");
    *n_out = 0;
    if (m->M == 0 || !(wi_local[2] > 0.0f)) return SDMM_OK;   // getDMM: no model, or cosTheta(wi) <= 0
    float w[kLearnedMaxComp], mm[3 * kLearnedMaxComp], cc[4 * kLearnedMaxComp];
    int n;
    {
        const DeviceFloatEnv env;
        float x[kLearnedMaxCond];
        x[0] = (float)std::acos((double)std::fmin(1.0f, wi_local[2]));
        for (int i = 0; i < m->C - 1; ++i) x[1 + i] = cond_rest[i];
        n = m->C == 2 ? learned_conditional<2>(rec, m->M, x, wi_local, keep, force, w, mm, cc)
                      : learned_conditional<3>(rec, m->M, x, wi_local, keep, force, w, mm, cc);
    }
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
    const DeviceFloatEnv env;
    if (u) {
        float o[3] = {0.0f, 0.0f, 1.0f};
        phong_sample(wi, params, rho, u[0], u[1], o, value, pdf);
        for (int a = 0; a < 3; ++a) wo[a] = o[a];
    } else {
        *pdf = phong_eval_pdf(wi, wo, params, rho, value);
    }
    return SDMM_OK;
}

int sdmm_bsdf_roughdielectric_host(const float* params, const float spec_trans[3], const float wi[3], const float* u,
                                   float wo[3], float value[3], float* pdf, float* eta_out) {
    if (!params || params[0] != (float)kBsdfDielectric || !spec_trans || !wi || !wo || !value || !pdf || !eta_out)
        return fail(SDMM_E_INVALID, "sdmm_bsdf_roughdielectric_host: invalid argument (params of a kind-4 BSDF)");
    const DeviceFloatEnv env;
    if (u) {
        float o[3];
        roughdielectric_sample(wi, params, spec_trans, u[0], u[1], u[2], o, value, pdf, eta_out);
        for (int a = 0; a < 3; ++a) wo[a] = o[a];
    } else {
        *pdf = roughdielectric_eval_pdf(wi, wo, params, spec_trans, value);
        *eta_out = roughdielectric_crossed_eta(wi, wo, params);
    }
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
    const DeviceFloatEnv env;
    if (u) {
        float o[3];
        smooth_sample(wi, params, st, u[0], o, value, pdf, eta_out);
        for (int a = 0; a < 3; ++a) wo[a] = o[a];
    } else {
        *pdf = smooth_eval_pdf(wi, wo, params, st, value, eta_out);
    }
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
    for (void* p : s->owned) (void)hipFree(p);
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
    HostScene hs;
    if (const int rc = build_host_scene(desc, "sdmm_scene_intersect_host", max_levels, &hs)) return rc;
    const DeviceFloatEnv env;
    for (int64_t i = 0; i < nq; ++i) prim[i] = closest(hs, mode, o + 3 * i, d + 3 * i, mint, maxt, t + i);
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
    HostScene hs;
    if (const int rc = build_host_scene(desc, "sdmm_scene_shading_host", 0, &hs)) return rc;
    // the scene as hit_normals reads it, on host arrays
    SceneDev S{};
    S.quads = hs.quads.data();
    S.n_quads = (int)hs.quads.size();
    S.hits = hs.mesh.hits.data();
    const MeshShade* shade = hs.mesh.shade.empty() ? nullptr : hs.mesh.shade.data();
    const DeviceFloatEnv env;
    for (int64_t i = 0; i < nq; ++i) {
        prim[i] = closest(hs, mode, o + 3 * i, d + 3 * i, mint, maxt, t + i);
        for (int a = 0; a < 3; ++a) ns[3 * i + a] = ng[3 * i + a] = 0.0f;
        if (prim[i] >= 0) hit_normals(S, shade, prim[i], o + 3 * i, d + 3 * i, ns + 3 * i, ng + 3 * i);
    }
    return SDMM_OK;
}

int sdmm_scene_texture(const sdmm_scene* s, int64_t nq, const float* const o[3], const float* const d[3], float mint,
                       float maxt, int mode, int32_t* prim, float* t, float* const uv[2], float* const rgb[3],
                       void* hip_stream) {
    if (!s || nq < 0 || (mode != 0 && mode != 1))
        return fail(SDMM_E_INVALID, "sdmm_scene_texture: invalid argument (mode 0 or 1)");
    if (nq == 0) return SDMM_OK;
    if (!o || !o[0] || !o[1] || !o[2] || !d || !d[0] || !d[1] || !d[2] || !prim || !t || !uv || !uv[0] || !uv[1] ||
        !rgb || !rgb[0] || !rgb[1] || !rgb[2])
        return fail(SDMM_E_INVALID, "sdmm_scene_texture: NULL plane");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(launch_scene_texture(s->S, s->T, nq, o, d, mint, maxt, mode, prim, t, uv, rgb, (hipStream_t)hip_stream));
    return SDMM_OK;
}

int sdmm_scene_texture_host(const sdmm_scene_desc* desc, int64_t nq, const float* o, const float* d, float mint,
                            float maxt, int mode, int32_t* prim, float* t, float* uv, float* rgb) {
    if (!desc || nq < 0 || (mode != 0 && mode != 1) || (nq > 0 && (!o || !d || !prim || !t || !uv || !rgb)))
        return fail(SDMM_E_INVALID, "sdmm_scene_texture_host: invalid argument (mode 0 or 1)");
    HostScene hs;
    if (const int rc = build_host_scene(desc, "sdmm_scene_texture_host", 0, &hs)) return rc;
    HostTextures ht;
    if (const int rc = prep_textures(desc, "sdmm_scene_texture_host", hs, &ht)) return rc;
    // (the uv table also for a mesh with neither mesh_uvs nor textures: the test's own u, v)
    if (hs.has_mesh && ht.mesh_uv.empty()) {
        ht.mesh_uv.assign(hs.mesh.tris.size(), MeshUV{});
        for (const MeshTri& T : hs.mesh.tris) ht.mesh_uv[(size_t)T.id].tri = T;
    }
    const int nquads = (int)hs.quads.size();
    const DeviceFloatEnv env;
    for (int64_t i = 0; i < nq; ++i) {
        prim[i] = closest(hs, mode, o + 3 * i, d + 3 * i, mint, maxt, t + i);
        uv[2 * i] = uv[2 * i + 1] = 0.0f;
        for (int a = 0; a < 3; ++a) rgb[3 * i + a] = 0.0f;
        if (prim[i] < 0) continue;
        hit_uv(hs.quads.data(), nquads, ht.mesh_uv.data(), prim[i], o + 3 * i, d + 3 * i, uv + 2 * i);
        const int qb = prim[i] >= nquads ? hs.mesh.hits[(size_t)(prim[i] - nquads)].bsdf : hs.quads[(size_t)prim[i]].bsdf;
        hit_reflectance<false>(desc->reflectance, ht.tex.data(), ht.textured ? desc->bsdf_texture : nullptr, qb,
                               uv + 2 * i, rgb + 3 * i);
    }
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
    const DeviceFloatEnv flush;
    for (int64_t i = 0; i < nq; ++i) env_eval<false>(env, d + 3 * i, rgb + 3 * i);
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
    HIP_TRY(launch_li_camera(s->S, s->P, s->N, s->T, path0, p->spp, p->seed, st));
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
        HIP_TRY(launch_li_query(s->S, s->P, s->Q, s->N, s->T, path0, b, p->max_depth > 0 ? p->max_depth : INT32_MAX, p->guided,
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
        HIP_TRY(launch_li_shade(s->S, s->P, s->Q, s->N, s->T, path0, b, p->rr_depth, h, p->seed, product && p->guided, st));
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
