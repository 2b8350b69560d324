/* sdmm_oracle_li.inc -- CPU ORACLE (test infrastructure only; included by
 * sdmm_oracle.c).  SDMMRenderer::Li (mitsuba/src/integrators/sdmm/
 * sdmm_proc.cpp:592-871) over an analytic scene of parallelograms (Mitsuba
 * rectangles; a cube is six) and an optional triangle mesh, with diffuse,
 * plastic, rough-conductor, Phong and rough-dielectric BSDFs and one-sided
 * area emitters -- the scenes the library's device Li renders
 * (sdmm_li_render) -- one path at a time, restated from the reference as
 * text:
 *
 *   :641-677   first intersection, emission seen directly (before any vertex)
 *   :649-691   rRec.depth 1 .. maxDepth-1 scatter; the depth cap (:684-685)
 *   :697-734   no NEE (the plugin's NEE block is compiled out), so the MIS
 *              weight of a BSDF-sampled emitter hit is 1 (:811-816)
 *   :275-508   sampleSurface: the leaf (STree.find, :314), no trained context
 *              -> BSDF only with h = 1 (:316-323); the conditional (:368),
 *              the BSDF/guide choice with heuristicConditionalWeight 0.5
 *              (:383-392); sampleProduct: the product with the material's
 *              learned BSDF (:327-381) and h = 0.3 (0.5 without a usable
 *              product); the guided direction's bsdf->eval / pdf (:456-507)
 *   :510-590   pdfSurface: pdf = h bsdfPdf + (1 - h) gmmPdf
 *   :759-780   a zero weight or a strict-normals violation ends the path
 *   :803-846   trace; recordRadiance of an emitter hit into every saved
 *              vertex (:615-637); the new vertex with clampedPdf = max(pdf,
 *              0.1), weight value / clampedPdf (:821-845) when the bounce is
 *              cacheable -- not a delta lobe of a BSDF sample (:764)
 *   :392-409   a plastic bounce (bsdfs/plastic.cpp, the Kitchen's delta +
 *              smooth BSDF): the guide is queried as for any BSDF with a
 *              smooth lobe (:297); a delta lobe chosen by the BSDF sample
 *              returns weight / h with pdf * h (:401-405), a smooth one
 *              (weight * pdf) / pdfSurface, the guide's direction the smooth
 *              lobe's eval / pdfSurface
 *   :858-868   Russian roulette once rRec.depth >= rrDepth
 *   :327-355   a rough conductor (bsdfs/roughconductor.cpp:296-462 over
 *              microfacet.h: Beckmann, isotropic alpha, sampleVisible =
 *              false, fresnelConductorExact with gray eta / k): its learned
 *              BSDF (getDMM, roughconductor.cpp:182-196) conditioned on
 *              (theta_i, alpha) -- a synthetic 4-lobe fit, the suite's
 *              learned files being LFS pointers -- then rotate_to_wo(wi) and
 *              the shading frame to world (:340-355), the product's
 *              non-diffuse branch; BSDF samples and the guide's direction
 *              under eval / pdf as for any smooth BSDF
 *   :327-355   a Phong BSDF (bsdf kind 3; bsdfs/phong.cpp:171-289, both
 *              components): li_phong_sample at the loop head, the guide's
 *              direction under li_phong_eval_pdf, handled like the conductor
 *              in every other respect (no delta lobe, every bounce cacheable);
 *              in a product bounce its learned SDMM5 (getDMM, phong.cpp:75-90)
 *              conditioned on (theta_i, max specular channel, log max(1,
 *              exponent)), pruned to 2 with component 1 (the diffuse one)
 *              forced -- li_learned_nd_conditional -- then rotate_to_wo
 *   a rough dielectric (bsdf kind 4; bsdfs/roughdielectric.cpp eval :317-395,
 *              pdf :397-469, sample :560-662 over microfacet.h; libcore/
 *              util.cpp fresnelDielectricExt :651-681, refract :767-772):
 *              li_roughdielectric_* in double between float inputs and outputs
 *              (the library's documented contract).  The restatement keeps
 *              the library's operation order, and with it the shape of
 *              csrc/bsdf_roughdielectric.h (also what a void sample leaves in
 *              wo), because every rounding of the double arithmetic has to
 *              agree for the Li comparison to be bitwise: "equals the host
 *              call bit for bit" therefore shows only that the two texts say
 *              the same, not that either is right.  The independent evidence
 *              is the float64 numpy restatement and the furnace albedo
 *              (tests/test_li_oracle_dielectric.py).  The one two-sided
 *              material: alive from either side, dead at wi . n == 0 or with
 *              reflectance and transmittance both zero; sampled in Frame(n) of
 *              the stored normal whatever the side, the lobe's uniform
 *              (sampler->next1D(), :601) dimension 7 of the bounce's stream;
 *              the guide's direction evaluated over the whole sphere, bRec.eta
 *              there what sample would have set (li_roughdielectric_crossed);
 *              a vertex saved inside the medium carries -n (sdmm_proc.cpp
 *              :765-767); in a product bounce getDMM (:198-211): none from
 *              inside (:199), else its SDMM5 at (theta_i, alpha, eta), pruned
 *              to 2, no forced component
 *   :604, :788 the path's relative index: eta = 1, times bRec.eta of every
 *              bounce; :864 the roulette's q = min(max(thr) eta^2, 0.95)
 *
 * Triangles: Triangle::rayIntersect (include/mitsuba/core/triangle.h:109-145)
 * in float -- li_tri_intersect -- over every triangle in a loop, no hierarchy;
 * the closest hit of li_intersect has t in (mint, maxt), the smallest t, on
 * exactly equal t the lowest primitive id, quads before triangles (primitive
 * n_quads + i is triangle i); face normals normalize((p1 - p0) x (p2 - p0)),
 * flipped on request; the scene box reaches over the mesh vertices.
 *
 * The product's lobes per table row, lM: the device gives every compact query
 * a row of its own with max(M, 2) lobes as soon as some quad or triangle of
 * the scene has a rough-conductor, a Phong or a rough-dielectric BSDF --
 * whether or not that BSDF carries a learned model (sdmm_scene_create sets
 * per_query_lobes from the BSDF kinds alone; extend_learned re-strides the
 * caller's rows, the extra lobes weight 0) -- and M lobes otherwise.
 * or_li_render follows that rule, so the component indices k * lM + j agree.
 *
 * Scene conventions (Mitsuba): diffuse BSDFs sample the cosine hemisphere
 * (warp::squareToCosineHemisphere, concentric map) in Frame(n) (Mitsuba's
 * coordinateSystem); f * cos / pdf = rho; a BSDF with rho = 0 (the light's) or
 * a back-side hit ends the path; emitters radiate Le on their normal side;
 * the perspective camera maps (1 - 2 sx) tan(fov/2) along x.  Random numbers
 * are the library's counter-based uniforms (or_rng_uniform,
 * sdmm_oracle_train.c): stream 0 the camera (dims 0-1 the pixel jitter),
 * stream 1 + b bounce b (dims 0-1 BSDF sample, 2 BSDF/guide choice, 3-5 the
 * guide sample, 6 roulette, 7 the dielectric's lobe) -- not Mitsuba's sampler,
 * which cannot be run here.  Float arithmetic with -ffp-contract=off; sin/cos
 * of the cosine map as the correctly rounded (float)f((double)x).
 *
 * The guide on each leaf is this oracle's conditional (or_conditional_*) and
 * product (or_product_*) on that leaf's parameters.  node_mix[v] NULL: the
 * node has no trained context.  Output layout as sdmm_li_render: image /
 * image_sqr planes [3][W*H]; vertex field f of vertex v of path p at
 * rec[(f * V + v) * P + p]; comps[b * P + p]: the guided query's component
 * index (-1 no valid conditional, -2 the BSDF sample was chosen, -9 no query);
 * hit_bsdf[b * P + p]: the BSDF bounce b scattered at (-1: none); inside[b * P
 * + p]: 1 where it met the surface from behind, 0 from the front, -1 none.
 *
 * Environment emitters (`constant`, lat-long `envmap`): li_env_eval below,
 * written from emitters/constant.cpp, envmap.cpp:380-393, :409 and mipmap.h
 * :497-596 and not from the library's csrc/envmap.h -- the two are compared
 * in tests/test_li_oracle_env.py.  A camera ray that hits nothing returns
 * env(d) with throughput 1 and no vertex (sdmm_proc.cpp:659-671); a bounce ray
 * that hits nothing sets value = env(wo) (:1047-1051), and radiance,
 * recordRadiance and the saved vertex's weight follow as for an emitter hit;
 * the path ends there, without a roulette draw.  escaped[(b + 1) * P + p]: 1
 * where bounce b's ray left the scene, 0 where it hit something, -1 no ray;
 * row 0 the camera ray.
 */
#include <pthread.h>

typedef struct {
    float p0[3], e1[3], e2[3], n[3], g1[3], g2[3];
    int bsdf, emitter;
} li_quad;

/* a triangle of the mesh: corner and edges (p1 - p0, p2 - p0), the unit face
 * normal normalize((p1 - p0) x (p2 - p0)) with the flip applied */
typedef struct {
    float p0[3], e1[3], e2[3], n[3];
    int bsdf, emitter;
} li_tri;

/* the environment emitter (Scene::getEnvironmentEmitter): none, `constant`
 * (emitters/constant.cpp) or a lat-long `envmap` (emitters/envmap.cpp) */
#define LI_ENV_NONE 0
#define LI_ENV_CONSTANT 1
#define LI_ENV_LATLONG 2
typedef struct {
    int kind;
    float rad[3];      /* constant: m_radiance */
    const float* px;   /* envmap: [h][w][3], row 0 the +y pole (MIP level 0) */
    int w, h;
    float scale;       /* envmap: m_scale */
    float inv[9];      /* envmap: the linear part of m_worldTransform's inverse, row major */
} li_env;

typedef struct {
    li_quad* quads;
    int nq;
    li_tri* tris;   /* primitive id of triangle i: nq + i */
    int nt;
    const float* refl;
    const float* bpar;   /* 8 per BSDF (include/sdmm_gpu.h bsdf_params); NULL: all diffuse */
    const float* lmodel; /* LI_L4_STRIDE per BSDF: [M, M SDMM4 records]; NULL: no learned models */
    const float* lmodel_nd; /* LI_ND_STRIDE per BSDF: [C, M, M records of LI_ND_REC(C)]; NULL: none */
    const float* rad;
    li_env env;
    float cam[12];
    float tanx, aspect, near_clip;
    int width, height;
    float smin[3], snorm;
} li_scene;

static float li_dot3(const float a[3], const float b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
static void li_cross3(const float a[3], const float b[3], float c[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

float or_rng_uniform(uint64_t seed, uint64_t path, uint32_t stream, uint32_t dim);
int or_stree_find(const float* mn, const float* mx, const int* child, const float p[3]);

/* rectangle / cube faces as parallelograms: normal = (e1 x e2) / |e1 x e2|,
 * flipped on request; dual vectors g1 = (e2 x n) / (e1 . (e2 x n)), g2 =
 * (n x e1) / (e2 . (n x e1)) with the unnormalised n.  The mesh (nt > 0):
 * triangle i over the vertices tri[3 i .. 3 i + 2], its face normal as above.
 * The scene box over the quads' corners and every mesh vertex
 * (getAABBWithoutCamera), spatialNormalization = its largest extent
 * (volpath_sdmm.cpp:375-393).  nq == 0 (a mesh alone) is a scene. */
static int li_geometry_build(li_scene* S, const float* quads, const int32_t* flip, const int32_t* bsdf, int nq,
                             const int32_t* emitter, const float* verts, int nverts, const int32_t* tri, int nt,
                             const int32_t* tri_bsdf, const int32_t* tri_emitter, const int32_t* tri_flip) {
    S->quads = (li_quad*)malloc(sizeof(li_quad) * (size_t)(nq > 0 ? nq : 1));
    S->nq = nq;
    S->tris = (li_tri*)malloc(sizeof(li_tri) * (size_t)(nt > 0 ? nt : 1));
    S->nt = nt;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int q = 0; q < nq; ++q) {
        li_quad* Q = &S->quads[q];
        const float* v = quads + 9 * q;
        for (int a = 0; a < 3; ++a) { Q->p0[a] = v[a]; Q->e1[a] = v[3 + a]; Q->e2[a] = v[6 + a]; }
        float n[3];
        li_cross3(Q->e1, Q->e2, n);
        const float len = sqrtf(li_dot3(n, n));
        if (!(len > 0.0f)) return 0;
        const float sg = (flip && flip[q]) ? -1.0f : 1.0f;
        for (int a = 0; a < 3; ++a) Q->n[a] = sg * n[a] / len;
        float a1[3], a2[3];
        li_cross3(Q->e2, n, a1);
        li_cross3(n, Q->e1, a2);
        const float s1 = li_dot3(Q->e1, a1), s2 = li_dot3(Q->e2, a2);
        for (int a = 0; a < 3; ++a) { Q->g1[a] = a1[a] / s1; Q->g2[a] = a2[a] / s2; }
        Q->bsdf = bsdf ? bsdf[q] : 0;
        Q->emitter = emitter ? emitter[q] : -1;
        for (int c = 0; c < 4; ++c)
            for (int a = 0; a < 3; ++a) {
                const float x = Q->p0[a] + ((c & 1) ? Q->e1[a] : 0.0f) + ((c & 2) ? Q->e2[a] : 0.0f);
                mn[a] = fminf(mn[a], x);
                mx[a] = fmaxf(mx[a], x);
            }
    }
    if (nt > 0)
        for (int i = 0; i < nverts; ++i)
            for (int a = 0; a < 3; ++a) {
                mn[a] = fminf(mn[a], verts[3 * i + a]);
                mx[a] = fmaxf(mx[a], verts[3 * i + a]);
            }
    for (int i = 0; i < nt; ++i) {
        li_tri* T = &S->tris[i];
        for (int k = 0; k < 3; ++k)
            if (tri[3 * i + k] < 0 || tri[3 * i + k] >= nverts) return 0;
        const float *p0 = verts + 3 * tri[3 * i], *p1 = verts + 3 * tri[3 * i + 1], *p2 = verts + 3 * tri[3 * i + 2];
        for (int a = 0; a < 3; ++a) { T->p0[a] = p0[a]; T->e1[a] = p1[a] - p0[a]; T->e2[a] = p2[a] - p0[a]; }
        float n[3];
        li_cross3(T->e1, T->e2, n);
        const float len = sqrtf(li_dot3(n, n));
        if (!(len > 0.0f)) return 0;
        const float sg = (tri_flip && tri_flip[i]) ? -1.0f : 1.0f;
        for (int a = 0; a < 3; ++a) T->n[a] = sg * n[a] / len;
        T->bsdf = tri_bsdf ? tri_bsdf[i] : 0;
        T->emitter = tri_emitter ? tri_emitter[i] : -1;
    }
    float norm = 0.0f;
    for (int a = 0; a < 3; ++a) norm = fmaxf(norm, mx[a] - mn[a]);
    for (int a = 0; a < 3; ++a) S->smin[a] = mn[a];
    S->snorm = norm;
    return 1;
}

static int li_scene_build(li_scene* S, const float* quads, const int32_t* flip, const int32_t* bsdf, int nq,
                          const float* refl, const float* bpar, const int32_t* emitter, const float* rad,
                          const float cam[16], float fov, float near_clip, int width, int height, const float* verts,
                          int nverts, const int32_t* tri, int nt, const int32_t* tri_bsdf,
                          const int32_t* tri_emitter, const int32_t* tri_flip) {
    if (!li_geometry_build(S, quads, flip, bsdf, nq, emitter, verts, nverts, tri, nt, tri_bsdf, tri_emitter,
                           tri_flip))
        return 0;
    S->refl = refl;
    S->bpar = bpar;
    S->rad = rad;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) S->cam[4 * r + c] = cam[4 * r + c];
    S->tanx = (float)tan(0.5 * (double)fov * 3.14159265358979323846 / 180.0);
    S->aspect = (float)width / (float)height;
    S->near_clip = near_clip > 0.0f ? near_clip : 1e-2f;
    S->width = width;
    S->height = height;
    return 1;
}

/* Triangle::rayIntersect (include/mitsuba/core/triangle.h:109-145): pvec = d x
 * e2, det = e1 . pvec (0: no hit), u = (tvec . pvec) / det in [0, 1], qvec =
 * tvec x e1, v = (d . qvec) / det >= 0 with u + v <= 1, t = (e2 . qvec) / det
 * -- each "/ det" a product with inv_det = 1 / det, as there */
static int li_tri_intersect(const li_tri* T, const float o[3], const float d[3], float* t) {
    float pvec[3], qvec[3];
    li_cross3(d, T->e2, pvec);
    const float det = li_dot3(T->e1, pvec);
    if (det == 0.0f) return 0;
    const float inv_det = 1.0f / det;
    const float tvec[3] = {o[0] - T->p0[0], o[1] - T->p0[1], o[2] - T->p0[2]};
    const float u = li_dot3(tvec, pvec) * inv_det;
    if (u < 0.0f || u > 1.0f) return 0;
    li_cross3(tvec, T->e1, qvec);
    const float v = li_dot3(d, qvec) * inv_det;
    if (v >= 0.0f && u + v <= 1.0f) {
        *t = li_dot3(T->e2, qvec) * inv_det;
        return 1;
    }
    return 0;
}

/* closest hit with t in (mint, maxt): the smallest t wins, on exactly equal t
 * the lowest primitive id -- every quad before every triangle.  Both loops
 * visit the ids in ascending order, so the strict t < tb alone keeps the
 * lowest id of a tie.  All the triangles in a loop: no traversal to get wrong. */
static int li_intersect(const li_scene* S, const float o[3], const float d[3], float mint, float maxt, float* t_hit) {
    int best = -1;
    float tb = maxt;
    for (int q = 0; q < S->nq; ++q) {
        const li_quad* Q = &S->quads[q];
        const float denom = li_dot3(d, Q->n);
        if (denom == 0.0f) continue;
        const float r0[3] = {Q->p0[0] - o[0], Q->p0[1] - o[1], Q->p0[2] - o[2]};
        const float t = li_dot3(r0, Q->n) / denom;
        if (!(t > mint && t < tb)) continue;
        const float r[3] = {o[0] + t * d[0] - Q->p0[0], o[1] + t * d[1] - Q->p0[1], o[2] + t * d[2] - Q->p0[2]};
        const float a = li_dot3(r, Q->g1), b = li_dot3(r, Q->g2);
        if (a < 0.0f || a > 1.0f || b < 0.0f || b > 1.0f) continue;
        tb = t;
        best = q;
    }
    for (int i = 0; i < S->nt; ++i) {
        float t;
        if (!li_tri_intersect(&S->tris[i], o, d, &t)) continue;
        if (!(t > mint && t < maxt)) continue;
        if (t < tb) {
            tb = t;
            best = S->nq + i;
        }
    }
    *t_hit = tb;
    return best;
}
/* the hit primitive's normal, BSDF and emitter */
static const float* li_prim_n(const li_scene* S, int q) { return q >= S->nq ? S->tris[q - S->nq].n : S->quads[q].n; }
static int li_prim_bsdf(const li_scene* S, int q) { return q >= S->nq ? S->tris[q - S->nq].bsdf : S->quads[q].bsdf; }
static int li_prim_emitter(const li_scene* S, int q) {
    return q >= S->nq ? S->tris[q - S->nq].emitter : S->quads[q].emitter;
}

/* ctypes entry for the tests: the closest hit of nr rays (o, d: nr x 3)
 * against the quads and the mesh; prim -1 and t = maxt without a hit */
int or_li_intersect(const float* quads, const int32_t* flip, int n_quads, const float* verts, int n_verts,
                    const int32_t* tri, int n_tris, int64_t nr, const float* o, const float* d, float mint,
                    float maxt, int32_t* prim, float* t) {
    FTZ_SCOPE;
    li_scene S;
    memset(&S, 0, sizeof(S));
    const int ok = li_geometry_build(&S, quads, flip, NULL, n_quads, NULL, verts, n_verts, tri, n_tris, NULL, NULL,
                                     NULL);
    if (ok)
        for (int64_t r = 0; r < nr; ++r) prim[r] = li_intersect(&S, o + 3 * r, d + 3 * r, mint, maxt, &t[r]);
    free(S.quads);
    free(S.tris);
    return ok ? 0 : -1;
}

/* ---- environment emitters: Emitter::evalEnvironment ----
 * constant.cpp: m_radiance whatever the ray.  envmap.cpp:380-393, :409 without
 * ray differentials (this Li has none): v = toWorld^-1 d (d as given, no
 * renormalisation); uv = (atan2(v.x, -v.z) INV_TWOPI, safe_acos(v.y) INV_PI);
 * MIPMap::evalBilinear(0, uv) (mipmap.h:575-596); times m_scale.  Float; atan2
 * and acos in double, rounded to float once. */

/* MIPMap::evalTexel on level 0 (mipmap.h:497-563) with the envmap's boundary
 * conditions: ERepeat along x (math::modulo, the positive remainder), EClamp
 * along y */
static const float* li_env_texel(const li_env* E, int x, int y) {
    if (x < 0 || x >= E->w) {
        x = x % E->w;
        if (x < 0) x += E->w;
    }
    if (y < 0 || y >= E->h) y = y < 0 ? 0 : E->h - 1;
    return E->px + 3 * ((size_t)y * (size_t)E->w + (size_t)x);
}

static void li_env_eval(const li_env* E, const float d[3], float out[3]) {
    out[0] = out[1] = out[2] = 0.0f;
    if (E->kind == LI_ENV_CONSTANT) {
        for (int ch = 0; ch < 3; ++ch) out[ch] = E->rad[ch];
        return;
    }
    if (E->kind != LI_ENV_LATLONG) return;
    float v[3];
    for (int r = 0; r < 3; ++r) v[r] = E->inv[3 * r] * d[0] + E->inv[3 * r + 1] * d[1] + E->inv[3 * r + 2] * d[2];
    /* math::safe_acos: acos(std::min(1.0f, std::max(-1.0f, y))); std::max(a, b) is a < b ? b : a and std::min(a,
     * b) is b < a ? b : a, so a NaN y becomes -1 */
    float yc = -1.0f < v[1] ? v[1] : -1.0f;
    yc = yc < 1.0f ? yc : 1.0f;
    const float uvx = (float)atan2((double)v[0], (double)-v[2]) * 0.15915494309189533577f;
    const float uvy = fl_acos(yc) * 0.31830988618379067154f;
    if (!isfinite(uvx) || !isfinite(uvy)) return;   /* evalBilinear's guard: Value(0) */
    const float u = uvx * (float)E->w - 0.5f, t = uvy * (float)E->h - 0.5f;
    const int xp = (int)floorf(u), yp = (int)floorf(t);   /* math::floorToInt */
    const float dx1 = u - (float)xp, dx2 = 1.0f - dx1;
    const float dy1 = t - (float)yp, dy2 = 1.0f - dy1;
    const float *a = li_env_texel(E, xp, yp), *b = li_env_texel(E, xp, yp + 1);
    const float *c = li_env_texel(E, xp + 1, yp), *e = li_env_texel(E, xp + 1, yp + 1);
    for (int ch = 0; ch < 3; ++ch)
        out[ch] = (a[ch] * dx2 * dy2 + b[ch] * dx2 * dy1 + c[ch] * dx1 * dy2 + e[ch] * dx1 * dy1) * E->scale;
}

/* the env fields of a description (the keys pkg.Scene reads) -> li_env; 0: not a valid emitter */
static int li_env_build(li_env* E, int kind, const float* radiance, const float* pixels, int w, int h, float scale,
                        const float* world_to_local) {
    memset(E, 0, sizeof(*E));
    E->kind = kind;
    if (kind == LI_ENV_NONE) return 1;
    if (kind == LI_ENV_CONSTANT) {
        if (!radiance) return 0;
        for (int ch = 0; ch < 3; ++ch) E->rad[ch] = radiance[ch];
        return 1;
    }
    if (kind != LI_ENV_LATLONG || !pixels || w < 1 || h < 1 || !world_to_local) return 0;
    E->px = pixels;
    E->w = w;
    E->h = h;
    E->scale = scale;
    for (int k = 0; k < 9; ++k) E->inv[k] = world_to_local[k];
    return 1;
}

/* ctypes entry for the tests: evalEnvironment of n directions (d, rgb: n x 3) */
int or_env_eval(int kind, const float* radiance, const float* pixels, int w, int h, float scale,
                const float* world_to_local, int64_t n, const float* d, float* rgb) {
    FTZ_SCOPE;
    li_env E;
    if (!li_env_build(&E, kind, radiance, pixels, w, h, scale, world_to_local)) return -1;
    for (int64_t i = 0; i < n; ++i) li_env_eval(&E, d + 3 * i, rgb + 3 * i);
    return 0;
}

/* fresnelDielectricExt (libcore/util.cpp:651-681), the reflectance */
static float li_fresnel(float cos_i, float eta) {
    if (eta == 1.0f) return 0.0f;
    const float scale = cos_i > 0.0f ? 1.0f / eta : eta;
    const float ct2 = 1.0f - (1.0f - cos_i * cos_i) * (scale * scale);
    if (ct2 <= 0.0f) return 1.0f;
    const float ci = fabsf(cos_i), ct = sqrtf(ct2);
    const float rs = (ci - eta * ct) / (ci + eta * ct);
    const float rp = (eta * ci - ct) / (eta * ci + ct);
    return 0.5f * (rs * rs + rp * rp);
}

/* SmoothPlastic probSpecular (plastic.cpp:339-342) */
static float li_prob_spec(float Fi, float ssw) {
    /* 0 / 0 -> 0 (NaN in the reference; both lobes carry no energy there) */
    const float num = Fi * ssw, den = num + (1.0f - Fi) * (1.0f - ssw);
    return den == 0.0f ? 0.0f : num / den;
}

/* ---- rough conductor (roughconductor.cpp, microfacet.h) ---- */
#define LI_PI_F 3.14159265358979323846f

/* fresnelConductorExact, Spectrum form (libcore/util.cpp:739-761), gray */
static float li_fresnel_conductor(float ci, float eta, float k) {
    const float ci2 = ci * ci, si2 = 1.0f - ci2, si4 = si2 * si2;
    const float t1 = eta * eta - k * k - si2;
    const float a2pb2 = sqrtf(fmaxf(0.0f, t1 * t1 + k * k * eta * eta * 4.0f));
    const float a = sqrtf(fmaxf(0.0f, (a2pb2 + t1) * 0.5f));
    const float term1 = a2pb2 + ci2, term2 = a * (2.0f * ci);
    const float rs2 = (term1 - term2) / (term1 + term2);
    const float term3 = a2pb2 * ci2 + si4, term4 = term2 * si2;
    const float rp2 = rs2 * (term3 - term4) / (term3 + term4);
    return 0.5f * (rp2 + rs2);
}
/* MicrofacetDistribution::eval, Beckmann (microfacet.h:191-233) */
static float li_beckmann_d(const float m[3], float alpha) {
    if (m[2] <= 0.0f) return 0.0f;
    const float ct2 = m[2] * m[2];
    const float ex = ((m[0] * m[0]) / (alpha * alpha) + (m[1] * m[1]) / (alpha * alpha)) / ct2;
    float r = (float)exp((double)-ex) / (LI_PI_F * alpha * alpha * ct2 * ct2);
    if (r * m[2] < 1e-20f) r = 0.0f;
    return r;
}
/* smithG1 (microfacet.h:477-518) */
static float li_beckmann_g1(const float v[3], const float m[3], float alpha) {
    if (li_dot3(v, m) * v[2] <= 0.0f) return 0.0f;
    const float tmp = 1.0f - v[2] * v[2];
    const float tan_t = tmp <= 0.0f ? 0.0f : fabsf(sqrtf(tmp) / v[2]);
    if (tan_t == 0.0f) return 1.0f;
    const float a = 1.0f / (alpha * tan_t);
    if (a >= 1.6f) return 1.0f;
    const float a2 = a * a;
    return (3.535f * a + 2.181f * a2) / (1.0f + 2.276f * a + 2.577f * a2);
}
/* RoughConductor::sample(bRec, pdf, sample), local frame, wi.z > 0: 0 = void */
static int li_conductor_sample(const float wi[3], const float* bp, float u0, float u1, float wo[3], float bw[3],
                               float* pdf) {
    const float alpha = bp[6];
    const float phi = (2.0f * LI_PI_F) * u1;
    const float sp = fl_sin(phi), cp = fl_cos(phi);
    const float a2 = alpha * alpha;
    const float tan2 = a2 * -fl_log(1.0f - u0);
    const float ct = 1.0f / sqrtf(1.0f + tan2);
    float mpdf = (1.0f - u0) / (LI_PI_F * alpha * alpha * ct * ct * ct);
    if (mpdf < 1e-20f) mpdf = 0.0f;
    const float st = sqrtf(fmaxf(0.0f, 1.0f - ct * ct));
    const float m[3] = {st * cp, st * sp, ct};
    *pdf = 0.0f;
    bw[0] = bw[1] = bw[2] = 0.0f;
    wo[0] = 0.0f; wo[1] = 0.0f; wo[2] = 1.0f;
    if (mpdf == 0.0f) return 0;
    const float dm = li_dot3(wi, m);
    for (int a = 0; a < 3; ++a) wo[a] = 2.0f * dm * m[a] - wi[a];
    if (wo[2] <= 0.0f) return 0;
    const float fr = li_fresnel_conductor(dm, bp[4], bp[5]);
    const float g = li_beckmann_g1(wi, m, alpha) * li_beckmann_g1(wo, m, alpha);
    const float weight = li_beckmann_d(m, alpha) * g * dm / (mpdf * wi[2]);
    for (int ch = 0; ch < 3; ++ch) bw[ch] = fr * bp[1 + ch] * weight;
    *pdf = mpdf / (4.0f * li_dot3(wo, m));
    return 1;
}
/* RoughConductor::eval (ESolidAngle) into f, returns pdf (roughconductor.cpp:302-366) */
static float li_conductor_eval_pdf(const float wi[3], const float wo[3], const float* bp, float f[3]) {
    f[0] = f[1] = f[2] = 0.0f;
    if (wi[2] <= 0.0f || wo[2] <= 0.0f) return 0.0f;
    const float alpha = bp[6];
    const float hs[3] = {wo[0] + wi[0], wo[1] + wi[1], wo[2] + wi[2]};
    const float rc = 1.0f / sqrtf(hs[0] * hs[0] + hs[1] * hs[1] + hs[2] * hs[2]);   /* normalize: v * (1/|v|) */
    const float H[3] = {hs[0] * rc, hs[1] * rc, hs[2] * rc};
    const float D = li_beckmann_d(H, alpha);
    if (D != 0.0f) {
        const float fr = li_fresnel_conductor(li_dot3(wi, H), bp[4], bp[5]);
        const float G = li_beckmann_g1(wi, H, alpha) * li_beckmann_g1(wo, H, alpha);
        const float model = D * G / (4.0f * wi[2]);
        for (int ch = 0; ch < 3; ++ch) f[ch] = fr * bp[1 + ch] * model;
    }
    return D * H[2] / (4.0f * fabsf(li_dot3(wo, H)));
}
/* The conductor's learned BSDF for local wi: getDMM (roughconductor.cpp:
 * 182-194) -- the material's SDMM4 (bsdf.h:310-314; records of 22 floats: w,
 * mean (theta, alpha, unit direction), 4x4 tangent covariance over (theta,
 * alpha, t1, t2) at the direction's Coordinates frame) conditioned on
 * (theta_i, alpha) with create_conditional_pruned(..., 2) -- then
 * rotate_to_wo(wi) (sdmm_proc.cpp:340-355).  sdmm-lib is absent; the reading
 * restated here (the library's csrc/learned_bsdf.h states the same):
 *   pi'_k = pi_k N(x; mu_c, S_cc) (Cholesky of S_cc; not PD: pi' = 0),
 *   shift = S_dc S_cc^-1 (x - mu_c), S'_dd = S_dd - S_dc S_cc^-1 S_cd (not
 *   PD: pi' = 0), mean' = exp_{mu_d}(shift), S'_dd re-expressed in
 *   Coordinates(mean') from mu_d's tangent axes parallel-transported along
 *   the geodesic; pruned to the `keep` largest pi' (ties: the lower index),
 *   renormalised; rotate_to_wo: R = Rz(azimuth of wi), mean R mean', the
 *   covariance re-expressed in Coordinates(R mean') from R's image of the
 *   Coordinates(mean') axes.  Returns the lobes written (0: no valid
 *   conditional -- getDMM false). */
#define LI_L4_MAX 8
#define LI_L4_REC 22
#define LI_L4_STRIDE (1 + LI_L4_MAX * LI_L4_REC)
#define LI_L4_KEEP 2
static void li_l4_cong(float b00, float b01, float b10, float b11, float s00, float s01, float s11, float c[3]) {
    const float t00 = b00 * s00 + b01 * s01, t01 = b00 * s01 + b01 * s11;
    const float t10 = b10 * s00 + b11 * s01, t11 = b10 * s01 + b11 * s11;
    c[0] = t00 * b00 + t01 * b01;
    c[1] = t00 * b10 + t01 * b11;
    c[2] = t10 * b10 + t11 * b11;
}
/* rotate_to_wo's rotation about the normal: cos / sin of wl's azimuth (1, 0 at the pole) */
static void li_l4_azimuth(const float wl[3], float* cr, float* sr) {
    const float sp2 = wl[0] * wl[0] + wl[1] * wl[1];
    *cr = 1.0f;
    *sr = 0.0f;
    if (sp2 > 0.0f) {
        const float rs = 1.0f / sqrtf(sp2);
        *cr = wl[0] * rs;
        *sr = wl[1] * rs;
    }
}
/* One conditioned component as a lobe (shared by the SDMM4 and the N-D
 * conditional): mean' = exp_{mu}(a0, a1), the covariance sc (s00, s01, s11 in
 * Coordinates(mu)) transported there, then rotate_to_wo by (cr, sr): mean[3],
 * cov[4] in Coordinates(mean). */
static void li_l4_lobe(const float* mu_d, float a0, float a1, const float sc[3], float cr, float sr, float* mean,
                       float* cov) {
    const float mu[3] = {mu_d[0], mu_d[1], mu_d[2]};
    float tm[9], td[9], tr[9], c1[3], c2[3];
    or_coordinates(mu, tm);
    float d[3] = {mu[0], mu[1], mu[2]};
    float e1[3] = {tm[0], tm[1], tm[2]}, e2[3] = {tm[3], tm[4], tm[5]};
    const float len2 = a0 * a0 + a1 * a1;
    if (len2 > 0.0f) {
        /* the geodesic from mu along u = shift / |shift|; mu's axes parallel-transported along it */
        const float len = sqrtf(len2);
        const float sn = (float)sin((double)len), cs = (float)cos((double)len);
        const float u0 = a0 / len, u1 = a1 / len;
        float u[3];
        for (int i = 0; i < 3; ++i) u[i] = u0 * tm[i] + u1 * tm[3 + i];
        for (int i = 0; i < 3; ++i) d[i] = cs * mu[i] + sn * u[i];
        for (int i = 0; i < 3; ++i) {
            const float g = (cs - 1.0f) * u[i] - sn * mu[i];
            e1[i] = tm[i] + u0 * g;
            e2[i] = tm[3 + i] + u1 * g;
        }
    }
    const float rn = 1.0f / sqrtf(li_dot3(d, d));
    for (int i = 0; i < 3; ++i) d[i] = d[i] * rn;
    or_coordinates(d, td);
    li_l4_cong(li_dot3(td, e1), li_dot3(td, e2), li_dot3(td + 3, e1), li_dot3(td + 3, e2), sc[0], sc[1], sc[2], c1);
    const float m[3] = {cr * d[0] - sr * d[1], sr * d[0] + cr * d[1], d[2]};
    or_coordinates(m, tr);
    const float r1[3] = {cr * td[0] - sr * td[1], sr * td[0] + cr * td[1], td[2]};
    const float r2[3] = {cr * td[3] - sr * td[4], sr * td[3] + cr * td[4], td[5]};
    li_l4_cong(li_dot3(tr, r1), li_dot3(tr, r2), li_dot3(tr + 3, r1), li_dot3(tr + 3, r2), c1[0], c1[1], c1[2], c2);
    mean[0] = m[0]; mean[1] = m[1]; mean[2] = m[2];
    cov[0] = c2[0]; cov[1] = c2[1]; cov[2] = c2[1]; cov[3] = c2[2];
}
static int li_learned_conditional(const float* rec, int M, float theta, float alpha, const float wl[3], int keep,
                                  float* w, float* mean, float* cov) {
    const float two_pi = 6.28318530717958647692f;
    float pw[LI_L4_MAX], sh[LI_L4_MAX][2], sc[LI_L4_MAX][3];
    int sel[LI_L4_MAX], n = 0;
    float sum = 0.0f;
    if (M > LI_L4_MAX) M = LI_L4_MAX;
    if (keep > LI_L4_MAX) keep = LI_L4_MAX;
    for (int k = 0; k < M; ++k) {
        const float* p = rec + LI_L4_REC * k;
        /* S_cc = [[p6 p7] [p10 p11]], S_cd = [[p8 p9] [p12 p13]], S_dc rows (p14 p15), (p18 p19), S_dd (p16 p17 p21) */
        pw[k] = 0.0f;
        sh[k][0] = sh[k][1] = 0.0f;
        sc[k][0] = sc[k][1] = sc[k][2] = 0.0f;
        if (!(p[6] > 0.0f)) continue;
        const float l00 = sqrtf(p[6]);
        const float l10 = p[7] / l00;
        const float rr = p[11] - l10 * l10;
        if (!(rr > 0.0f)) continue;
        const float l11 = sqrtf(rr);
        const float z0 = (theta - p[1]) / l00;
        const float z1 = ((alpha - p[2]) - l10 * z0) / l11;
        const float q = z0 * z0 + z1 * z1;
        const float dens = (float)exp((double)(-0.5f * q)) / (two_pi * (l00 * l11));
        const float y1 = z1 / l11;
        const float y0 = (z0 - l10 * y1) / l00;
        sh[k][0] = p[14] * y0 + p[15] * y1;
        sh[k][1] = p[18] * y0 + p[19] * y1;
        const float g00 = p[8] / l00, g10 = (p[12] - l10 * g00) / l11;
        const float g01 = p[9] / l00, g11 = (p[13] - l10 * g01) / l11;
        const float s00 = p[16] - (g00 * g00 + g10 * g10);
        const float s01 = p[17] - (g00 * g01 + g10 * g11);
        const float s11 = p[21] - (g01 * g01 + g11 * g11);
        if (!(s00 > 0.0f) || !(s00 * s11 - s01 * s01 > 0.0f)) continue;
        sc[k][0] = s00;
        sc[k][1] = s01;
        sc[k][2] = s11;
        pw[k] = p[0] * dens;
    }
    for (int slot = 0; slot < keep; ++slot) {
        int best = -1;
        for (int k = 0; k < M; ++k) {
            int taken = 0;
            for (int t = 0; t < n; ++t) taken = taken || sel[t] == k;
            if (taken || !(pw[k] > 0.0f)) continue;
            if (best < 0 || pw[k] > pw[best]) best = k;
        }
        if (best < 0) break;
        sel[n++] = best;
        sum += pw[best];
    }
    if (n == 0 || !(sum > 0.0f) || !(sum < INFINITY)) return 0;
    float cr, sr;
    li_l4_azimuth(wl, &cr, &sr);
    for (int j = 0; j < n; ++j) {
        const int k = sel[j];
        w[j] = pw[k] / sum;
        li_l4_lobe(rec + LI_L4_REC * k + 3, sh[k][0], sh[k][1], sc[k], cr, sr, mean + 3 * j, cov + 4 * j);
    }
    return n;
}

/* ctypes entry for the tests: the lobes of one SDMM4 (M records) at local wi */
int or_learned4_conditional(const float* rec, int M, float alpha, const float wl[3], int keep, float* w, float* mean,
                            float* cov) {
    FTZ_SCOPE;
    if (!(wl[2] > 0.0f)) return 0;
    return li_learned_conditional(rec, M, fl_acos(fminf(1.0f, wl[2])), alpha, wl, keep, w, mean, cov);
}

/* A learned BSDF over a condition of dimension C (2: an SDMM4, 3: the SDMM5 of
 * bsdf.h:316-324, Phong's on (theta_i, specWeight, log exponent), phong.cpp:
 * 75-90), conditioned on x[C] at local wi.  One record: the weight, the C
 * condition means, the unit direction, the (C+2)x(C+2) covariance row-major
 * over (c_0 .. c_{C-1}, t1, t2).  The reading of the absent sdmm-lib calls, as
 * above, with
 *   S_cc = L L^T by a lower Cholesky that reads the upper triangle; a pivot
 *   not > 0: pi' = 0; pi' = pi N(x; mu_c, S_cc) with the normaliser
 *   (2 pi)^(C/2) prod l_ii; z = L^-1 (x - mu_c), y = L^-T z; shift = S_dc y;
 *   G = L^-1 S_cd, S'_dd = S_dd - G^T G (not PD: pi' = 0);
 *   keep 1..8: create_conditional_pruned -- the `keep` largest pi' (ties: the
 *   lower index); force >= 0 (the five-argument call's diffuse_component): that
 *   component, if valid (force < M, pi' > 0) and not chosen before the last
 *   place, takes the last place; keep 0: create_conditional, every pi' > 0 in
 *   model order; renormalised.  Lobes as li_l4_lobe.  Returns the lobes
 *   written, 0: no valid conditional. */
#define LI_ND_MAXC 3
#define LI_ND_REC(C) (1 + ((C) + 3) + ((C) + 2) * ((C) + 2))
#define LI_ND_STRIDE (2 + LI_L4_MAX * LI_ND_REC(LI_ND_MAXC))   /* per BSDF: [C, M, records] */
#define LI_PHONG_FORCE 1                                        /* phong.cpp:76 */
static int li_learned_nd_conditional(const float* rec, int C, int M, const float* x, const float wl[3], int keep,
                                     int force, float* w, float* mean, float* cov) {
    if (C < 2 || C > LI_ND_MAXC) return 0;
    const int D = C + 2, R = LI_ND_REC(C);
    const float norm = (float)pow(2.0 * OR_PI, 0.5 * (double)C);
    float pw[LI_L4_MAX], sh[LI_L4_MAX][2], sc[LI_L4_MAX][3];
    if (M > LI_L4_MAX) M = LI_L4_MAX;
    if (keep > LI_L4_MAX) keep = LI_L4_MAX;
    for (int k = 0; k < M; ++k) {
        const float* p = rec + R * k;
        const float* S = p + 1 + C + 3;
        float L[LI_ND_MAXC][LI_ND_MAXC], z[LI_ND_MAXC], y[LI_ND_MAXC], G[LI_ND_MAXC][2];
        pw[k] = 0.0f;
        sh[k][0] = sh[k][1] = 0.0f;
        sc[k][0] = sc[k][1] = sc[k][2] = 0.0f;
        /* row i of L from the rows above it */
        float ldet = 1.0f;
        int ok = 1;
        for (int i = 0; i < C && ok; ++i) {
            for (int j = 0; j < i; ++j) {
                float a = S[D * j + i];
                for (int l = 0; l < j; ++l) a = a - L[i][l] * L[j][l];
                L[i][j] = a / L[j][j];
            }
            float piv = S[D * i + i];
            for (int l = 0; l < i; ++l) piv = piv - L[i][l] * L[i][l];
            if (!(piv > 0.0f)) { ok = 0; break; }
            L[i][i] = sqrtf(piv);
            ldet = ldet * L[i][i];
        }
        if (!ok) continue;
        float maha = 0.0f;
        for (int i = 0; i < C; ++i) {
            float a = x[i] - p[1 + i];
            for (int l = 0; l < i; ++l) a = a - L[i][l] * z[l];
            z[i] = a / L[i][i];
            maha = maha + z[i] * z[i];
        }
        const float dens = (float)exp((double)(-0.5f * maha)) / (norm * ldet);
        for (int i = C - 1; i >= 0; --i) {
            float a = z[i];
            for (int l = i + 1; l < C; ++l) a = a - L[l][i] * y[l];
            y[i] = a / L[i][i];
        }
        for (int t = 0; t < 2; ++t) {
            const float* row = S + D * (C + t);   /* S_dc, tangent row t */
            float a = row[0] * y[0];
            for (int l = 1; l < C; ++l) a = a + row[l] * y[l];
            sh[k][t] = a;
            for (int i = 0; i < C; ++i) {         /* column t of G = L^-1 S_cd */
                float b = S[D * i + C + t];
                for (int l = 0; l < i; ++l) b = b - L[i][l] * G[l][t];
                G[i][t] = b / L[i][i];
            }
        }
        float g00 = G[0][0] * G[0][0], g01 = G[0][0] * G[0][1], g11 = G[0][1] * G[0][1];
        for (int l = 1; l < C; ++l) {
            g00 = g00 + G[l][0] * G[l][0];
            g01 = g01 + G[l][0] * G[l][1];
            g11 = g11 + G[l][1] * G[l][1];
        }
        const float s00 = S[D * C + C] - g00, s01 = S[D * C + C + 1] - g01, s11 = S[D * (C + 1) + C + 1] - g11;
        if (!(s00 > 0.0f) || !(s00 * s11 - s01 * s01 > 0.0f)) continue;
        sc[k][0] = s00;
        sc[k][1] = s01;
        sc[k][2] = s11;
        pw[k] = p[0] * dens;
    }
    int sel[LI_L4_MAX], n = 0;
    float sum = 0.0f;
    if (keep == 0) {
        for (int k = 0; k < M; ++k)
            if (pw[k] > 0.0f) { sel[n++] = k; sum += pw[k]; }
    } else {
        int pending = force >= 0 && force < M && pw[force] > 0.0f;   /* the forced component still to be placed */
        for (int slot = 0; slot < keep; ++slot) {
            int best = -1;
            if (pending && slot == keep - 1) {
                best = force;
            } else {
                for (int k = 0; k < M; ++k) {
                    int taken = 0;
                    for (int t = 0; t < n; ++t) taken = taken || sel[t] == k;
                    if (taken || !(pw[k] > 0.0f)) continue;
                    if (best < 0 || pw[k] > pw[best]) best = k;
                }
            }
            if (best < 0) break;
            if (best == force) pending = 0;
            sel[n++] = best;
            sum += pw[best];
        }
    }
    if (n == 0 || !(sum > 0.0f) || !(sum < INFINITY)) return 0;
    float cr, sr;
    li_l4_azimuth(wl, &cr, &sr);
    for (int j = 0; j < n; ++j) {
        const int k = sel[j];
        w[j] = pw[k] / sum;
        li_l4_lobe(rec + R * k + 1 + C, sh[k][0], sh[k][1], sc[k], cr, sr, mean + 3 * j, cov + 4 * j);
    }
    return n;
}

/* ctypes entry for the tests: the lobes of one model (M records of LI_ND_REC(C)
 * floats) at local wi and the condition (theta_i, x_rest[0 .. C-2]) */
int or_learned_nd_conditional(const float* rec, int C, int M, const float* x_rest, const float wl[3], int keep,
                              int force, float* w, float* mean, float* cov) {
    FTZ_SCOPE;
    if (C < 2 || C > LI_ND_MAXC || M <= 0 || !(wl[2] > 0.0f)) return 0;
    float x[LI_ND_MAXC];
    x[0] = fl_acos(fminf(1.0f, wl[2]));
    for (int i = 1; i < C; ++i) x[i] = x_rest[i - 1];
    return li_learned_nd_conditional(rec, C, M, x, wl, keep, force, w, mean, cov);
}

/* Mitsuba coordinateSystem (s, t) of n */
static void li_frame(const float n[3], float s[3], float t[3]) {
    if (fabsf(n[0]) > fabsf(n[1])) {
        const float inv = 1.0f / sqrtf(n[0] * n[0] + n[2] * n[2]);
        t[0] = n[2] * inv; t[1] = 0.0f; t[2] = -n[0] * inv;
    } else {
        const float inv = 1.0f / sqrtf(n[1] * n[1] + n[2] * n[2]);
        t[0] = 0.0f; t[1] = n[2] * inv; t[2] = -n[1] * inv;
    }
    s[0] = t[1] * n[2] - t[2] * n[1];
    s[1] = t[2] * n[0] - t[0] * n[2];
    s[2] = t[0] * n[1] - t[1] * n[0];
}

/* warp::squareToCosineHemisphere (concentric disk, z guarded to 1e-10) */
static void li_cosine_hemisphere(float u0, float u1, float w[3]) {
    const float r1 = 2.0f * u0 - 1.0f, r2 = 2.0f * u1 - 1.0f;
    float r, phi;
    if (r1 == 0.0f && r2 == 0.0f) {
        r = 0.0f; phi = 0.0f;
    } else if (r1 * r1 > r2 * r2) {
        r = r1; phi = (float)(OR_PI / 4.0) * (r2 / r1);
    } else {
        r = r2; phi = (float)(OR_PI / 2.0) - (r1 / r2) * (float)(OR_PI / 4.0);
    }
    const float sp = fl_sin(phi), cp = fl_cos(phi);
    w[0] = r * cp;
    w[1] = r * sp;
    float z = sqrtf(fmaxf(0.0f, 1.0f - w[0] * w[0] - w[1] * w[1]));
    if (z == 0.0f) z = 1e-10f;
    w[2] = z;
}

/* ---- modified Phong (bsdfs/phong.cpp), local frame, both components ----
 * bp: [1..3] specularReflectance, [4] exponent, [5] m_specularSamplingWeight;
 * rho: diffuseReflectance.  pow as (float)pow((double)x, (double)y). */
static float fl_pow(float x, float y) { return (float)pow((double)x, (double)y); }
/* Phong::eval (ESolidAngle, :171-196) into f; returns Phong::pdf (:198-230) */
static float li_phong_eval_pdf(const float wi[3], const float wo[3], const float* bp, const float rho[3], float f[3]) {
    const float inv_pi = 0.31830988618379067154f, inv_two_pi = 0.15915494309189533577f;
    f[0] = f[1] = f[2] = 0.0f;
    if (wi[2] <= 0.0f || wo[2] <= 0.0f) return 0.0f;
    const float n = bp[4];
    const float refl[3] = {-wi[0], -wi[1], wi[2]};   /* reflect(wi) (:167-169) */
    const float ca = li_dot3(wo, refl);
    float lobe = 0.0f, spec_prob = 0.0f;
    if (ca > 0.0f) {
        const float can = fl_pow(ca, n);
        lobe = (n + 2.0f) * inv_two_pi * can;               /* :188 */
        spec_prob = can * (n + 1.0f) / (2.0f * LI_PI_F);    /* :217-218 */
    }
    for (int ch = 0; ch < 3; ++ch) f[ch] = (bp[1 + ch] * lobe + rho[ch] * inv_pi) * wo[2];
    return bp[5] * spec_prob + (1.0f - bp[5]) * (inv_pi * wo[2]);   /* :222-223 */
}
/* Phong::sample(bRec, pdf, sample) (:232-289), wi.z > 0: wo, eval / pdf into
 * bw and the pdf; 0: void (weight 0, pdf 0; wo as far as it was formed).  The
 * specular component is chosen with u0 <= weight && weight > 0 (the library's
 * documented deviation: with weight 0 the reference divides 0 by 0 at u0 = 0). */
static int li_phong_sample(const float wi[3], const float* bp, const float rho[3], float u0, float u1, float wo[3],
                           float bw[3], float* pdf) {
    const float n = bp[4], ssw = bp[5];
    *pdf = 0.0f;
    bw[0] = bw[1] = bw[2] = 0.0f;
    if (ssw > 0.0f && u0 <= ssw) {
        const float ux = u0 / ssw;                               /* :247 */
        const float refl[3] = {-wi[0], -wi[1], wi[2]};
        /* a lobe about (0, 0, 1) (:260-267), then Frame(R).toWorld (:270) */
        const float cos_a = fl_pow(u1, 1.0f / (n + 1.0f));
        const float sin_a = sqrtf(1.0f - fl_pow(u1, 2.0f / (n + 1.0f)));
        const float phi = (2.0f * LI_PI_F) * ux;
        const float lx = sin_a * fl_cos(phi), ly = sin_a * fl_sin(phi);
        float s[3], t[3];
        li_frame(refl, s, t);
        for (int a = 0; a < 3; ++a) wo[a] = s[a] * lx + t[a] * ly + refl[a] * cos_a;
        if (wo[2] <= 0.0f) return 0;                             /* :274-275 */
    } else {
        li_cosine_hemisphere((u0 - ssw) / (1.0f - ssw), u1, wo); /* :249-250, :277 */
    }
    float f[3];
    const float p = li_phong_eval_pdf(wi, wo, bp, rho, f);
    if (p == 0.0f) return 0;                                     /* :285-286 */
    const float rp = 1.0f / p;   /* Spectrum / Float: times the reciprocal */
    for (int ch = 0; ch < 3; ++ch) bw[ch] = f[ch] * rp;
    *pdf = p;
    return 1;
}
/* ctypes entry for the tests: u given -> the sample (s_wo, s_weight, s_pdf);
 * wo_eval given -> eval and pdf there (e_f, e_pdf) */
void or_bsdf_phong(const float* bp, const float rho[3], const float wi[3], const float* u, const float* wo_eval,
                   float s_wo[3], float s_weight[3], float* s_pdf, float e_f[3], float* e_pdf) {
    FTZ_SCOPE;
    if (u) {
        s_wo[0] = 0.0f; s_wo[1] = 0.0f; s_wo[2] = 1.0f;
        li_phong_sample(wi, bp, rho, u[0], u[1], s_wo, s_weight, s_pdf);
    }
    if (wo_eval) *e_pdf = li_phong_eval_pdf(wi, wo_eval, bp, rho, e_f);
}

/* ---- rough dielectric (bsdfs/roughdielectric.cpp over microfacet.h), local
 * frame, bsdf kind 4: isotropic Beckmann, sampleVisible = false, both
 * components, ERadiance.  bp: [1..3] specularReflectance, [4] eta = intIOR /
 * extIOR, [5] 1 / eta, [6] alpha; st: specularTransmittance (the BSDF's
 * reflectance row).  wi.z < 0 is a hit from inside.  The library's numeric
 * contract: float in and out, double in between without contraction, exp / log
 * / sincos in double, each result rounded to float once; the reference's float
 * constants (1e-20f, smithG1's coefficients) keep their float values. ---- */
extern void sincos(double x, double* s, double* c);
#define LID_PI 3.14159265358979323846
static double lid_dot3(const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
/* fresnelDielectricExt with cosThetaT (libcore/util.cpp:651-681), eta != 1:
 * cos_t signed against cos_i, 0 at a total internal reflection */
static double lid_fresnel(double cos_i, double eta, double* cos_t) {
    const double scale = cos_i > 0.0 ? 1.0 / eta : eta;
    const double ct2 = 1.0 - (1.0 - cos_i * cos_i) * (scale * scale);
    if (ct2 <= 0.0) {
        *cos_t = 0.0;
        return 1.0;
    }
    const double ci = fabs(cos_i), ct = sqrt(ct2);
    const double rs = (ci - eta * ct) / (ci + eta * ct);
    const double rp = (eta * ci - ct) / (eta * ci + ct);
    *cos_t = cos_i > 0.0 ? -ct : ct;
    return 0.5 * (rs * rs + rp * rp);
}
/* MicrofacetDistribution::eval, Beckmann (microfacet.h:191-233) */
static double lid_beckmann_d(const double m[3], double alpha) {
    if (m[2] <= 0.0) return 0.0;
    const double ct2 = m[2] * m[2];
    const double ex = ((m[0] * m[0]) / (alpha * alpha) + (m[1] * m[1]) / (alpha * alpha)) / ct2;
    double r = exp(-ex) / (LID_PI * alpha * alpha * ct2 * ct2);
    if (r * m[2] < (double)1e-20f) r = 0.0;
    return r;
}
/* smithG1 (microfacet.h:477-518) */
static double lid_beckmann_g1(const double v[3], const double m[3], double alpha) {
    if (lid_dot3(v, m) * v[2] <= 0.0) return 0.0;
    const double tmp = 1.0 - v[2] * v[2];
    const double tan_t = tmp <= 0.0 ? 0.0 : fabs(sqrt(tmp) / v[2]);
    if (tan_t == 0.0) return 1.0;
    const double a = 1.0 / (alpha * tan_t);
    if (a >= (double)1.6f) return 1.0;
    const double a2 = a * a;
    return ((double)3.535f * a + (double)2.181f * a2) / (1.0 + (double)2.276f * a + (double)2.577f * a2);
}
/* sampleAll (microfacet.h:287-395): the microfacet normal of (u0, u1), its density (0 below 1e-20) */
static double lid_beckmann_sample(double alpha, double u0, double u1, double m[3]) {
    const double phi = (2.0 * LID_PI) * u1;
    double sp, cp;
    sincos(phi, &sp, &cp);
    const double a2 = alpha * alpha;
    const double tan2 = a2 * -log(1.0 - u0);
    const double ct = 1.0 / sqrt(1.0 + tan2);
    double mpdf = (1.0 - u0) / (LID_PI * alpha * alpha * ct * ct * ct);
    if (mpdf < (double)1e-20f) mpdf = 0.0;
    const double st = sqrt(fmax(0.0, 1.0 - ct * ct));
    m[0] = st * cp; m[1] = st * sp; m[2] = ct;
    return mpdf;
}
/* the Walter trick (roughdielectric.cpp:453-458, :492-498): the sampling distribution's alpha */
static double lid_sample_alpha(double alpha, double cos_i) { return alpha * (1.2 - 0.2 * sqrt(fabs(cos_i))); }
/* bRec.eta as sample sets it (:615, :633) for a given pair of directions: 1
 * on reflection, eta entering (wi.z > 0), 1 / eta leaving */
static float li_roughdielectric_crossed(const float wi[3], const float wo[3], const float* bp) {
    if ((double)wi[2] * (double)wo[2] > 0.0) return 1.0f;
    return wi[2] > 0.0f ? bp[4] : bp[5];
}
/* RoughDielectric::eval (ESolidAngle, :317-395) into f; returns RoughDielectric::pdf
 * (:397-469).  wo on either side; wi.z == 0: both 0 (:318). */
static float li_roughdielectric_eval_pdf(const float wi_[3], const float wo_[3], const float* bp, const float st[3],
                                         float f[3]) {
    f[0] = f[1] = f[2] = 0.0f;
    if (wi_[2] == 0.0f) return 0.0f;
    const double wi[3] = {wi_[0], wi_[1], wi_[2]}, wo[3] = {wo_[0], wo_[1], wo_[2]};
    const double eta = bp[4], inv_eta = bp[5], alpha = bp[6];
    const int reflect = wi[2] * wo[2] > 0.0;
    const double e = wi[2] > 0.0 ? eta : inv_eta;
    double hs[3], H[3];
    for (int a = 0; a < 3; ++a) hs[a] = reflect ? wo[a] + wi[a] : wi[a] + wo[a] * e;   /* :340-349 */
    const double rc = 1.0 / sqrt(hs[0] * hs[0] + hs[1] * hs[1] + hs[2] * hs[2]);
    for (int a = 0; a < 3; ++a) H[a] = hs[a] * rc;
    if (copysign(1.0, H[2]) < 0.0)                                                     /* H *= signum(cosTheta(H)) */
        for (int a = 0; a < 3; ++a) H[a] = -H[a];
    const double wi_h = lid_dot3(wi, H), wo_h = lid_dot3(wo, H);
    double cos_t;
    const double F = lid_fresnel(wi_h, eta, &cos_t);
    const double sqrt_denom = wi_h + e * wo_h;
    const double D = lid_beckmann_d(H, alpha);
    if (D != 0.0) {
        const double G = lid_beckmann_g1(wi, H, alpha) * lid_beckmann_g1(wo, H, alpha);
        if (reflect) {
            const double value = F * D * G / (4.0 * fabs(wi[2]));                      /* :373-377 */
            for (int ch = 0; ch < 3; ++ch) f[ch] = (float)((double)bp[1 + ch] * value);
        } else {
            const double value = ((1.0 - F) * D * G * e * e * wi_h * wo_h) / (wi[2] * sqrt_denom * sqrt_denom);
            const double factor = wi[2] > 0.0 ? inv_eta : eta;                         /* ERadiance (:389-393) */
            const double v = fabs(value * factor * factor);
            for (int ch = 0; ch < 3; ++ch) f[ch] = (float)((double)st[ch] * v);
        }
    }
    const double dwh_dwo = reflect ? 1.0 / (4.0 * wo_h) : (e * e * wo_h) / (sqrt_denom * sqrt_denom);
    double prob = lid_beckmann_d(H, lid_sample_alpha(alpha, wi[2])) * H[2];
    prob *= reflect ? F : (1.0 - F);
    return (float)fabs(prob * dwh_dwo);
}
/* RoughDielectric::sample(bRec, pdf, sample) (:560-662); u2: the sampler's
 * next1D() for the lobe, reflection when u2 <= F.  0: void (weight 0, pdf 0,
 * eta 1; wo as far as it was formed) -- microfacet pdf 0, a failed side check,
 * cosThetaT == 0 (refract, libcore/util.cpp:767-772), wi.z == 0. */
static int li_roughdielectric_sample(const float wi_[3], const float* bp, const float st[3], float u0, float u1,
                                     float u2, float wo_[3], float bw[3], float* pdf, float* eta_out) {
    const double eta = bp[4], inv_eta = bp[5], alpha = bp[6];
    *pdf = 0.0f;
    *eta_out = 1.0f;
    bw[0] = bw[1] = bw[2] = 0.0f;
    wo_[0] = 0.0f; wo_[1] = 0.0f; wo_[2] = 1.0f;
    if (wi_[2] == 0.0f) return 0;
    const double wi[3] = {wi_[0], wi_[1], wi_[2]};
    double m[3], wo[3];
    const double mpdf = lid_beckmann_sample(lid_sample_alpha(alpha, wi[2]), (double)u0, (double)u1, m);
    if (mpdf == 0.0) return 0;
    const double dm = lid_dot3(wi, m);
    double cos_t;
    const double F = lid_fresnel(dm, eta, &cos_t);
    const int reflect = (double)u2 <= F;
    double p, dwh_dwo, scale = 1.0;
    float crossed = 1.0f;
    const float* tint;
    if (reflect) {
        p = mpdf * F;
        for (int a = 0; a < 3; ++a) wo[a] = 2.0 * dm * m[a] - wi[a];
        for (int a = 0; a < 3; ++a) wo_[a] = (float)wo[a];
        if (wi[2] * wo[2] <= 0.0 || wo_[2] == 0.0f) return 0;
        tint = bp + 1;
        dwh_dwo = 1.0 / (4.0 * lid_dot3(wo, m));
    } else {
        p = mpdf * (1.0 - F);
        if (cos_t == 0.0) return 0;
        const double er = cos_t < 0.0 ? inv_eta : eta;     /* refract(wi, m, eta, cosThetaT) */
        const double k = dm * er + cos_t;
        for (int a = 0; a < 3; ++a) wo[a] = m[a] * k - wi[a] * er;
        for (int a = 0; a < 3; ++a) wo_[a] = (float)wo[a];
        crossed = cos_t < 0.0 ? bp[4] : bp[5];
        if (wi[2] * wo[2] >= 0.0 || wo_[2] == 0.0f) return 0;
        const double factor = cos_t < 0.0 ? inv_eta : eta;
        tint = st;
        scale = factor * factor;
        const double wo_m = lid_dot3(wo, m), ce = (double)crossed;
        const double sqrt_denom = dm + ce * wo_m;
        dwh_dwo = (ce * ce * wo_m) / (sqrt_denom * sqrt_denom);
    }
    const double g = lid_beckmann_g1(wi, m, alpha) * lid_beckmann_g1(wo, m, alpha);
    const double weight = fabs(lid_beckmann_d(m, alpha) * g * dm / (mpdf * wi[2]));
    for (int ch = 0; ch < 3; ++ch) bw[ch] = (float)(((double)tint[ch] * scale) * weight);
    *pdf = (float)fabs(p * dwh_dwo);
    *eta_out = crossed;
    return 1;
}
/* ctypes entry for the tests: u (3) given -> the sample (s_wo, s_weight,
 * s_pdf, eta); wo_eval given -> eval, pdf and the crossed index there */
void or_bsdf_roughdielectric(const float* bp, const float st[3], const float wi[3], const float* u,
                             const float* wo_eval, float s_wo[3], float s_weight[3], float* s_pdf, float e_f[3],
                             float* e_pdf, float* eta_out) {
    FTZ_SCOPE;
    if (u) li_roughdielectric_sample(wi, bp, st, u[0], u[1], u[2], s_wo, s_weight, s_pdf, eta_out);
    if (wo_eval) {
        *e_pdf = li_roughdielectric_eval_pdf(wi, wo_eval, bp, st, e_f);
        *eta_out = li_roughdielectric_crossed(wi, wo_eval, bp);
    }
}

typedef struct {
    const li_scene* S;
    const float *mn, *mx;
    const int* child;
    const or_mixture* const* node_mix;
    int guided, spp, max_depth, rr_depth, V, product;
    float h;
    uint64_t seed;
    int64_t path0, P;
    /* sampleProduct: learned-BSDF rows per scene BSDF */
    const float *bw, *bmean, *bcov;
    const uint8_t* bdiff;
    int M, Kmax;
    int lM;   /* the product's lobes per row: max(M, 2) with a conductor or a Phong BSDF on some quad, else M */
    float* rec;
    int32_t* nv;
    float* L;        /* P x 3 radiance */
    int32_t* comps;  /* bounces x P */
    int32_t* hit_bsdf;   /* bounces x P, optional: the BSDF a live bounce scattered at (-1: none) */
    int32_t* inside;     /* bounces x P, optional: 1 a live bounce met its surface from behind (wi . n < 0), 0
                            from the front, -1 no live bounce */
    int rr_eta_one;      /* tests only: roulette with the path's relative index taken as 1 */
    int32_t* escaped;    /* (bounces + 1) x P, optional: row 0 the camera ray, row b + 1 bounce b's ray: 1 it left
                            the scene (the environment, if any, was evaluated), 0 it hit something, -1 no ray */
    int bounces;
} li_job;

#define LI_REC(J, f, v, p) (J)->rec[((int64_t)(f) * (J)->V + (v)) * (J)->P + (p)]

/* one bounce's guided query against the leaf mixture m at condition c:
 * comp / direction / pdf / h as the device wavefront returns them */
static int li_guide_query(const li_job* J, const or_mixture* m, or_conditional* cd, or_product* pr, const float c[3],
                          const float u[3], const float bdir[3], int mode_bsdf, float choice, int material,
                          const float F[9], int glossy, const float* gw, const float* gm, const float* gc, float d[3],
                          float* pdf, float* hq) {
    *hq = J->h;
    if (!or_conditional_create(m, c, cd)) { *pdf = 0.0f; *hq = 1.0f; return -1; }
    if (!J->product) {
        if (mode_bsdf) {
            *pdf = or_conditional_pdf(m, cd, bdir);
            d[0] = bdir[0]; d[1] = bdir[1]; d[2] = bdir[2];
            return -2;
        }
        const int s = or_conditional_sample(m, cd, u, d);
        *pdf = or_conditional_pdf(m, cd, d);
        return cd->index[s];
    }
    int used = 0;
    if (glossy > 0) {
        /* the conductor's own lobes for this bounce (the render's query row) */
        used = or_product_create(m, cd, gw, gm, gc, J->lM, F, 0, pr);
    } else if (glossy == 0 && material >= 0 && J->M > 0) {
        /* the material's row, re-strided to lM lobes (the extra ones weight 0) */
        float rw[64], rm[64 * 3], rc[64 * 4];
        for (int l = 0; l < J->lM; ++l) {
            const int in = l < J->M;
            rw[l] = in ? J->bw[(size_t)material * J->M + l] : 0.0f;
            for (int a = 0; a < 3; ++a) rm[3 * l + a] = in ? J->bmean[((size_t)material * J->M + l) * 3 + a] : 0.0f;
            for (int a = 0; a < 4; ++a) rc[4 * l + a] = in ? J->bcov[((size_t)material * J->M + l) * 4 + a] : 0.0f;
        }
        used = or_product_create(m, cd, rw, rm, rc, J->lM, F, J->bdiff ? J->bdiff[material] : 0, pr);
    }
    *hq = used ? 0.3f : 0.5f;
    if (choice <= *hq) {
        *pdf = used ? or_product_pdf(pr, bdir) : or_conditional_pdf(m, cd, bdir);
        d[0] = bdir[0]; d[1] = bdir[1]; d[2] = bdir[2];
        return -2;
    }
    if (used) {
        const int s = or_product_sample(pr, u, d);
        *pdf = or_product_pdf(pr, d);
        return pr->comp[s];
    }
    const int s = or_conditional_sample(m, cd, u, d);
    *pdf = or_conditional_pdf(m, cd, d);
    return cd->index[s];
}

static void li_path(const li_job* J, int64_t i, or_conditional* cd, or_product* pr) {
    const li_scene* S = J->S;
    const float kEps = 1e-4f, kInvPi = 0.31830988618379067154f;
    const uint64_t gp = (uint64_t)(J->path0 + i);
    /* camera (:641-677) */
    const int64_t pix = (int64_t)gp / J->spp;
    const int px = (int)(pix % S->width), py = (int)(pix / S->width);
    const float sx = ((float)px + or_rng_uniform(J->seed, gp, 0, 0)) / (float)S->width;
    const float sy = ((float)py + or_rng_uniform(J->seed, gp, 0, 1)) / (float)S->height;
    float l[3] = {(1.0f - 2.0f * sx) * S->tanx, (1.0f - 2.0f * sy) * S->tanx / S->aspect, 1.0f};
    const float inv = 1.0f / sqrtf(li_dot3(l, l));
    for (int a = 0; a < 3; ++a) l[a] *= inv;
    float d[3], o[3];
    for (int r = 0; r < 3; ++r) {
        d[r] = S->cam[4 * r] * l[0] + S->cam[4 * r + 1] * l[1] + S->cam[4 * r + 2] * l[2];
        o[r] = S->cam[4 * r + 3];
    }
    const float dn = 1.0f / sqrtf(li_dot3(d, d));
    for (int a = 0; a < 3; ++a) d[a] *= dn;
    float t;
    int q = li_intersect(S, o, d, S->near_clip / l[2], INFINITY, &t);
    float thr[3] = {1.0f, 1.0f, 1.0f}, Li[3] = {0.0f, 0.0f, 0.0f}, p[3] = {0.0f, 0.0f, 0.0f};
    int nv = 0;
    float eta = 1.0f;   /* the path's relative index (:604) */
    if (q >= 0) {
        const int qe = li_prim_emitter(S, q);
        for (int a = 0; a < 3; ++a) p[a] = o[a] + t * d[a];
        if (qe >= 0 && -li_dot3(d, li_prim_n(S, q)) > 0.0f)
            for (int ch = 0; ch < 3; ++ch) Li[ch] = S->rad[3 * qe + ch];
    } else {
        /* no intersection: the environment seen directly, throughput 1, no vertex (:659-671) */
        li_env_eval(&S->env, d, Li);
    }
    if (J->escaped) J->escaped[i] = q >= 0 ? 0 : 1;
    int depth = q >= 0 ? 1 : -1;
    for (int b = 0; b < J->bounces; ++b) {
        int32_t comp_out = -9, bsdf_out = -1, inside_out = -1, escaped_out = -1;
        if (depth >= 0) {
            /* loop head (:684-691), sampleSurface (:275-421) */
            int live = !(J->max_depth >= 0 && depth >= J->max_depth);
            const int qbsdf = li_prim_bsdf(S, q);
            const float* n = li_prim_n(S, q);
            const float* rho = S->refl + 3 * qbsdf;
            const float* bp = S->bpar ? S->bpar + 8 * qbsdf : NULL;
            const int plastic = bp && bp[0] == 1.0f;
            const int conductor = bp && bp[0] == 2.0f;
            const int phong = bp && bp[0] == 3.0f;
            const int dielectric = bp && bp[0] == 4.0f;
            const int zero_spec = !(plastic || conductor || phong || dielectric) ||
                                  (bp[1] == 0.0f && bp[2] == 0.0f && bp[3] == 0.0f);
            /* (a dielectric's reflectance row is its specularTransmittance) */
            const int zero_diff = conductor || (rho[0] == 0.0f && rho[1] == 0.0f && rho[2] == 0.0f);
            const float wi[3] = {-d[0], -d[1], -d[2]};
            /* a rough dielectric scatters from either side: it is dead only at wi . n == 0 */
            const float cos_i = li_dot3(wi, n);
            const int side = dielectric ? (cos_i > 0.0f || cos_i < 0.0f) : cos_i > 0.0f;
            const int inside = dielectric && cos_i < 0.0f;   /* cosTheta(bRec.wi) < 0 */
            if (live && (!side || (zero_diff && zero_spec)))
                live = 0;
            if (!live) {
                depth = -1;
            } else {
                const uint32_t stream = 1u + (uint32_t)b;
                bsdf_out = qbsdf;
                inside_out = cos_i < 0.0f ? 1 : 0;
                const float c[3] = {(p[0] - S->smin[0]) / S->snorm, (p[1] - S->smin[1]) / S->snorm,
                                    (p[2] - S->smin[2]) / S->snorm};
                float s[3], tt[3], w[3];
                li_frame(n, s, tt);
                /* the BSDF sample (plastic: SmoothPlastic::sample, plastic.cpp:378-420) */
                int delta = 0;
                float bw[3] = {0.0f, 0.0f, 0.0f}, bpdf = 0.0f, Fi = 0.0f, ps = 0.0f;
                float bcrossed = 1.0f;   /* bRec.eta of the BSDF sample */
                if (plastic) {
                    const float wl[3] = {li_dot3(wi, s), li_dot3(wi, tt), li_dot3(wi, n)};
                    Fi = li_fresnel(wl[2], bp[4]);
                    ps = li_prob_spec(Fi, bp[7]);
                    const float u0 = or_rng_uniform(J->seed, gp, stream, 0), u1 = or_rng_uniform(J->seed, gp, stream, 1);
                    if (u0 < ps) {
                        delta = 1;
                        w[0] = -wl[0]; w[1] = -wl[1]; w[2] = wl[2];
                        const float rs = 1.0f / ps;   /* Spectrum / Float: times the reciprocal */
                        for (int ch = 0; ch < 3; ++ch) bw[ch] = bp[1 + ch] * Fi * rs;
                        bpdf = ps;
                    } else {
                        li_cosine_hemisphere((u0 - ps) / (1.0f - ps), u1, w);
                        const float Fo = li_fresnel(w[2], bp[4]);
                        const float rd = 1.0f / (1.0f - bp[6]);
                        const float k = bp[5] * (1.0f - Fi) * (1.0f - Fo) / (1.0f - ps);
                        for (int ch = 0; ch < 3; ++ch) bw[ch] = rho[ch] * rd * k;
                        bpdf = (1.0f - ps) * (kInvPi * w[2]);
                    }
                } else if (conductor) {
                    const float wl[3] = {li_dot3(wi, s), li_dot3(wi, tt), li_dot3(wi, n)};
                    li_conductor_sample(wl, bp, or_rng_uniform(J->seed, gp, stream, 0),
                                        or_rng_uniform(J->seed, gp, stream, 1), w, bw, &bpdf);
                } else if (phong) {
                    const float wl[3] = {li_dot3(wi, s), li_dot3(wi, tt), li_dot3(wi, n)};
                    li_phong_sample(wl, bp, rho, or_rng_uniform(J->seed, gp, stream, 0),
                                    or_rng_uniform(J->seed, gp, stream, 1), w, bw, &bpdf);
                } else if (dielectric) {
                    /* Frame(n) of the stored normal whatever the side; the lobe's uniform
                     * (sampler->next1D(), roughdielectric.cpp:601) is dimension 7 */
                    const float wl[3] = {li_dot3(wi, s), li_dot3(wi, tt), li_dot3(wi, n)};
                    li_roughdielectric_sample(wl, bp, rho, or_rng_uniform(J->seed, gp, stream, 0),
                                              or_rng_uniform(J->seed, gp, stream, 1),
                                              or_rng_uniform(J->seed, gp, stream, 7), w, bw, &bpdf, &bcrossed);
                } else {
                    li_cosine_hemisphere(or_rng_uniform(J->seed, gp, stream, 0),
                                         or_rng_uniform(J->seed, gp, stream, 1), w);
                }
                const float bdir[3] = {s[0] * w[0] + tt[0] * w[1] + n[0] * w[2],
                                       s[1] * w[0] + tt[1] * w[1] + n[1] * w[2],
                                       s[2] * w[0] + tt[2] * w[1] + n[2] * w[2]};
                const float u[3] = {or_rng_uniform(J->seed, gp, stream, 3), or_rng_uniform(J->seed, gp, stream, 4),
                                    or_rng_uniform(J->seed, gp, stream, 5)};
                const float choice = or_rng_uniform(J->seed, gp, stream, 2);
                const int mode_bsdf = (!J->guided || choice <= J->h) ? 1 : 0;
                float h = J->h, gd[3] = {0.0f, 0.0f, 0.0f}, gpdf = 0.0f;
                int comp = -1;
                if (J->guided) {
                    const int node = or_stree_find(J->mn, J->mx, J->child, c);
                    const or_mixture* m = node >= 0 ? J->node_mix[node] : NULL;
                    if (m) {
                        const float F[9] = {s[0], tt[0], n[0], s[1], tt[1], n[1], s[2], tt[2], n[2]};
                        float hq, gw[64], gm[64 * 3], gc[64 * 4];
                        /* 1: the conductor's / Phong's own lobes, -1: such a BSDF without a valid getDMM */
                        int glossy = 0;
                        if (conductor && J->product) {
                            const float wl[3] = {li_dot3(wi, s), li_dot3(wi, tt), li_dot3(wi, n)};
                            const float* lm = J->S->lmodel ? J->S->lmodel + (size_t)LI_L4_STRIDE * qbsdf : NULL;
                            const int LM = lm ? (int)lm[0] : 0;
                            int kept = 0;
                            if (LM > 0)
                                kept = li_learned_conditional(lm + 1, LM, fl_acos(fminf(1.0f, wl[2])), bp[6], wl,
                                                              LI_L4_KEEP, gw, gm, gc);
                            for (int l = kept; l < J->lM; ++l) gw[l] = 0.0f;
                            glossy = kept > 0 ? 1 : -1;
                        } else if (phong && J->product) {
                            /* Phong::getDMM (phong.cpp:75-90): the SDMM5 at (theta_i, the largest
                             * specular channel, log max(1, exponent)), pruned to 2 with the diffuse
                             * component kept */
                            const float wl[3] = {li_dot3(wi, s), li_dot3(wi, tt), li_dot3(wi, n)};
                            const float* lm =
                                J->S->lmodel_nd ? J->S->lmodel_nd + (size_t)LI_ND_STRIDE * qbsdf : NULL;
                            const int LM = lm ? (int)lm[1] : 0;
                            int kept = 0;
                            if (LM > 0) {
                                const float x[3] = {fl_acos(fminf(1.0f, wl[2])), fmaxf(bp[1], fmaxf(bp[2], bp[3])),
                                                    fl_log(fmaxf(1.0f, bp[4]))};
                                kept = li_learned_nd_conditional(lm + 2, (int)lm[0], LM, x, wl, LI_L4_KEEP,
                                                                 LI_PHONG_FORCE, gw, gm, gc);
                            }
                            for (int l = kept; l < J->lM; ++l) gw[l] = 0.0f;
                            glossy = kept > 0 ? 1 : -1;
                        } else if (dielectric && J->product) {
                            /* RoughDielectric::getDMM (roughdielectric.cpp:198-211): none from
                             * inside (cosTheta(wi) <= 0, :199); else the SDMM5 at (theta_i, alpha,
                             * eta), pruned to 2, no forced component */
                            const float wl[3] = {li_dot3(wi, s), li_dot3(wi, tt), li_dot3(wi, n)};
                            const float* lm =
                                J->S->lmodel_nd ? J->S->lmodel_nd + (size_t)LI_ND_STRIDE * qbsdf : NULL;
                            const int LM = lm ? (int)lm[1] : 0;
                            int kept = 0;
                            if (LM > 0 && wl[2] > 0.0f) {
                                const float x[3] = {fl_acos(fminf(1.0f, wl[2])), bp[6], bp[4]};
                                kept = li_learned_nd_conditional(lm + 2, (int)lm[0], LM, x, wl, LI_L4_KEEP, -1, gw, gm,
                                                                 gc);
                            }
                            for (int l = kept; l < J->lM; ++l) gw[l] = 0.0f;
                            glossy = kept > 0 ? 1 : -1;
                        }
                        comp = li_guide_query(J, m, cd, pr, c, u, bdir, mode_bsdf, choice, qbsdf, F, glossy, gw,
                                              gm, gc, gd, &gpdf, &hq);
                        if (J->product && comp != -1) h = hq;
                    }
                    comp_out = comp;
                }
                /* the rest of sampleSurface / pdfSurface (:392-507, :587-589) */
                float wo[3], weight[3], mis_pdf;
                int cacheable = 1;
                float crossed = 1.0f;   /* bRec.eta of the direction taken */
                if (plastic && comp != -1 && comp != -2) {
                    /* the guide's direction: the smooth lobe's eval / pdfSurface */
                    wo[0] = gd[0]; wo[1] = gd[1]; wo[2] = gd[2];
                    const float cos_o = li_dot3(wo, n);
                    const int zero = (wo[0] == 0.0f && wo[1] == 0.0f && wo[2] == 0.0f) || !isfinite(cos_o);
                    const int up = !zero && cos_o > 0.0f;
                    const float cpdf = kInvPi * cos_o;
                    const float bsdf_pdf = up ? cpdf * (1.0f - ps) : 0.0f;
                    mis_pdf = bsdf_pdf > 0.0f ? h * bsdf_pdf + (1.0f - h) * gpdf : 0.0f;
                    const float Fo = up ? li_fresnel(cos_o, bp[4]) : 0.0f;
                    const float rd = 1.0f / (1.0f - bp[6]);
                    const float k = cpdf * bp[5] * (1.0f - Fi) * (1.0f - Fo);
                    for (int ch = 0; ch < 3; ++ch) {
                        const float f = up ? rho[ch] * rd * k : 0.0f;
                        weight[ch] = mis_pdf == 0.0f ? 0.0f : f * (1.0f / mis_pdf);
                    }
                } else if (plastic) {
                    wo[0] = bdir[0]; wo[1] = bdir[1]; wo[2] = bdir[2];
                    cacheable = !delta;
                    if (comp == -1) {
                        mis_pdf = bpdf;
                        for (int ch = 0; ch < 3; ++ch) weight[ch] = bw[ch];
                    } else if (delta) {
                        mis_pdf = bpdf * h;
                        const float rh = 1.0f / h;
                        for (int ch = 0; ch < 3; ++ch) weight[ch] = bw[ch] * rh;
                    } else {
                        mis_pdf = bpdf > 0.0f ? h * bpdf + (1.0f - h) * gpdf : 0.0f;
                        for (int ch = 0; ch < 3; ++ch) weight[ch] = mis_pdf == 0.0f ? 0.0f : (bw[ch] * bpdf) * (1.0f / mis_pdf);
                    }
                } else if (conductor || phong || dielectric) {
                    if (comp == -1 || comp == -2) {
                        wo[0] = bdir[0]; wo[1] = bdir[1]; wo[2] = bdir[2];
                        crossed = bcrossed;
                        if (comp == -1) {
                            mis_pdf = bpdf;
                            for (int ch = 0; ch < 3; ++ch) weight[ch] = bw[ch];
                        } else {
                            mis_pdf = bpdf > 0.0f ? h * bpdf + (1.0f - h) * gpdf : 0.0f;
                            for (int ch = 0; ch < 3; ++ch)
                                weight[ch] = mis_pdf == 0.0f ? 0.0f : (bw[ch] * bpdf) * (1.0f / mis_pdf);
                        }
                    } else {
                        wo[0] = gd[0]; wo[1] = gd[1]; wo[2] = gd[2];
                        const float wil[3] = {li_dot3(wi, s), li_dot3(wi, tt), li_dot3(wi, n)};
                        const float wol[3] = {li_dot3(wo, s), li_dot3(wo, tt), li_dot3(wo, n)};
                        const int zero = (wo[0] == 0.0f && wo[1] == 0.0f && wo[2] == 0.0f) || !isfinite(wol[2]);
                        float f[3] = {0.0f, 0.0f, 0.0f};
                        /* (a dielectric: over the whole sphere; bRec.eta is what sample would
                         * have set for this direction -- eval leaves it unset) */
                        const float bsdf_pdf = zero         ? 0.0f
                                               : phong      ? li_phong_eval_pdf(wil, wol, bp, rho, f)
                                               : dielectric ? li_roughdielectric_eval_pdf(wil, wol, bp, rho, f)
                                                            : li_conductor_eval_pdf(wil, wol, bp, f);
                        if (dielectric) crossed = li_roughdielectric_crossed(wil, wol, bp);
                        mis_pdf = bsdf_pdf > 0.0f ? h * bsdf_pdf + (1.0f - h) * gpdf : 0.0f;
                        for (int ch = 0; ch < 3; ++ch) weight[ch] = mis_pdf == 0.0f ? 0.0f : f[ch] * (1.0f / mis_pdf);
                    }
                } else if (comp == -1) {
                    wo[0] = bdir[0]; wo[1] = bdir[1]; wo[2] = bdir[2];
                    mis_pdf = kInvPi * li_dot3(wo, n);
                    for (int ch = 0; ch < 3; ++ch) weight[ch] = rho[ch];
                } else if (comp == -2) {
                    wo[0] = bdir[0]; wo[1] = bdir[1]; wo[2] = bdir[2];
                    const float bsdf_pdf = kInvPi * li_dot3(wo, n);
                    mis_pdf = bsdf_pdf > 0.0f ? h * bsdf_pdf + (1.0f - h) * gpdf : 0.0f;
                    for (int ch = 0; ch < 3; ++ch) weight[ch] = mis_pdf == 0.0f ? 0.0f : (rho[ch] * bsdf_pdf) * (1.0f / mis_pdf);
                } else {
                    wo[0] = gd[0]; wo[1] = gd[1]; wo[2] = gd[2];
                    const float cos_o = li_dot3(wo, n);
                    const int zero = (wo[0] == 0.0f && wo[1] == 0.0f && wo[2] == 0.0f) || !isfinite(cos_o);
                    const float bsdf_pdf = (!zero && cos_o > 0.0f) ? kInvPi * cos_o : 0.0f;
                    mis_pdf = bsdf_pdf > 0.0f ? h * bsdf_pdf + (1.0f - h) * gpdf : 0.0f;
                    for (int ch = 0; ch < 3; ++ch)
                        weight[ch] = mis_pdf == 0.0f ? 0.0f : (rho[ch] * (kInvPi * cos_o)) * (1.0f / mis_pdf);
                }
                const float cos_o = li_dot3(wo, n);
                if ((weight[0] == 0.0f && weight[1] == 0.0f && weight[2] == 0.0f) || !(cos_o * cos_o > 0.0f) ||
                    !isfinite(weight[0] + weight[1] + weight[2])) {
                    depth = -1;
                } else {
                    for (int ch = 0; ch < 3; ++ch) thr[ch] = thr[ch] * weight[ch];
                    /* trace, look for an emitter (:803-819) */
                    const float oo[3] = {p[0], p[1], p[2]};
                    float th;
                    const int qh = li_intersect(S, oo, wo, kEps, INFINITY, &th);
                    float value[3] = {0.0f, 0.0f, 0.0f};
                    if (qh >= 0) {
                        const int he = li_prim_emitter(S, qh);
                        if (he >= 0 && -li_dot3(wo, li_prim_n(S, qh)) > 0.0f)
                            for (int ch = 0; ch < 3; ++ch) value[ch] = S->rad[3 * he + ch];
                    } else {
                        /* intersected nothing: value = env->evalEnvironment(ray) (:1047-1051) */
                        li_env_eval(&S->env, wo, value);
                    }
                    escaped_out = qh >= 0 ? 0 : 1;
                    if (value[0] != 0.0f || value[1] != 0.0f || value[2] != 0.0f) {
                        const float radv[3] = {thr[0] * value[0], thr[1] * value[1], thr[2] * value[2]};
                        for (int ch = 0; ch < 3; ++ch) Li[ch] += radv[ch];
                        for (int v = 0; v < nv; ++v) {   /* recordRadiance (:628-637) */
                            const float vp = LI_REC(J, 6, v, i);
                            for (int ch = 0; ch < 3; ++ch) {
                                const float vt = LI_REC(J, 3 + ch, v, i);
                                if (vt > kEps) LI_REC(J, ch, v, i) += radv[ch] / (vt * vp);
                            }
                        }
                    }
                    if (cacheable && nv < J->V) {   /* the saved vertex (:764, :821-845) */
                        const float clamped = fmaxf(mis_pdf, 0.1f);
                        const float inv_pdf = 1.0f / clamped;
                        for (int ch = 0; ch < 3; ++ch) {
                            LI_REC(J, ch, nv, i) = value[ch] * inv_pdf;
                            LI_REC(J, 3 + ch, nv, i) = thr[ch];
                        }
                        LI_REC(J, 6, nv, i) = clamped;
                        for (int a = 0; a < 3; ++a) {
                            LI_REC(J, 7 + a, nv, i) = c[a];
                            LI_REC(J, 10 + a, nv, i) = wo[a];
                            /* inside the medium the vertex carries -n (:765-767) */
                            LI_REC(J, 13 + a, nv, i) = inside ? -n[a] : n[a];
                        }
                        ++nv;
                    }
                    int alive = qh >= 0;
                    eta = eta * crossed;   /* eta *= bRec.eta (:788) */
                    if (depth >= J->rr_depth && alive) {   /* Russian roulette (:858-868) */
                        /* q = min(throughput.max() * eta * eta, 0.95) (:864) */
                        const float re = J->rr_eta_one ? 1.0f : eta;
                        const float qq = fminf(fmaxf(thr[0], fmaxf(thr[1], thr[2])) * re * re, 0.95f);
                        if (or_rng_uniform(J->seed, gp, 1u + (uint32_t)b, 6) >= qq) alive = 0;
                        else for (int ch = 0; ch < 3; ++ch) thr[ch] /= qq;
                    }
                    d[0] = wo[0]; d[1] = wo[1]; d[2] = wo[2];
                    if (alive) {
                        for (int a = 0; a < 3; ++a) p[a] = oo[a] + th * wo[a];
                        q = qh;
                    }
                    depth = alive ? depth + 1 : -1;
                }
            }
        }
        if (J->comps) J->comps[(int64_t)b * J->P + i] = comp_out;
        if (J->hit_bsdf) J->hit_bsdf[(int64_t)b * J->P + i] = bsdf_out;
        if (J->inside) J->inside[(int64_t)b * J->P + i] = inside_out;
        if (J->escaped) J->escaped[(int64_t)(b + 1) * J->P + i] = escaped_out;
    }
    J->nv[i] = nv;
    for (int ch = 0; ch < 3; ++ch) J->L[3 * i + ch] = Li[ch];
}

typedef struct {
    const li_job* J;
    int64_t a, b;
} li_range;

static void* li_worker(void* arg) {
    FTZ_SCOPE;
    const li_range* R = (const li_range*)arg;
    or_conditional cd;
    or_product pr;
    const int K = R->J->Kmax > 0 ? R->J->Kmax : 1;
    cond_alloc(&cd, K);
    prod_alloc(&pr, K * (R->J->lM > 0 ? R->J->lM : 1));
    for (int64_t i = R->a; i < R->b; ++i) li_path(R->J, i, &cd, &pr);
    prod_free(&pr);
    cond_free(&cd);
    return NULL;
}

/* One render pass of spp samples for pixels [pix_begin, pix_end) on nthreads
 * host threads (paths split in contiguous ranges; every path is independent).
 * Returns 0 on success. */
int or_li_render(const float* quads, const int32_t* flip, const int32_t* bsdf, int n_quads, const float* refl,
                 const float* bsdf_params, const int32_t* emitter, const float* rad, const float cam[16], float fov, float near_clip, int width,
                 int height, const float* mn, const float* mx, const int* child, const or_mixture* const* node_mix,
                 int guided, int spp, int max_depth, int rr_depth, float h, int V, uint64_t seed, int64_t pix_begin,
                 int64_t pix_end, int product, const float* bw, const float* bmean, const float* bcov,
                 const uint8_t* bdiff, int M, int Kmax, float* image, float* image_sqr, float* rec, int32_t* nv,
                 int32_t* comps, int nthreads, const float* learned_models, const float* learned_models_nd,
                 int32_t* hit_bsdf, const float* mesh_vertices, int n_mesh_vertices, const int32_t* triangles,
                 int n_triangles, const int32_t* tri_bsdf, const int32_t* tri_emitter, const int32_t* tri_flip,
                 int32_t* inside, int rr_eta_one, int env_kind, const float* env_radiance, const float* env_pixels,
                 int env_width, int env_height, float env_scale, const float* env_world_to_local,
                 int32_t* escaped) {
    FTZ_SCOPE;
    li_scene S;
    memset(&S, 0, sizeof(S));
    if (!li_env_build(&S.env, env_kind, env_radiance, env_pixels, env_width, env_height, env_scale,
                      env_world_to_local))
        return -1;
    if (!li_scene_build(&S, quads, flip, bsdf, n_quads, refl, bsdf_params, emitter, rad, cam, fov, near_clip, width,
                        height, mesh_vertices, n_mesh_vertices, triangles, n_triangles, tri_bsdf, tri_emitter,
                        tri_flip)) {
        free(S.quads);
        free(S.tris);
        return -1;
    }
    S.lmodel = learned_models;   /* LI_L4_STRIDE floats per BSDF, NULL: none */
    S.lmodel_nd = learned_models_nd;   /* LI_ND_STRIDE floats per BSDF, NULL: none */
    const int64_t npix = pix_end - pix_begin, P = npix * spp;
    li_job J;
    memset(&J, 0, sizeof(J));
    J.S = &S;
    J.mn = mn; J.mx = mx; J.child = child; J.node_mix = node_mix;
    J.guided = guided; J.spp = spp; J.max_depth = max_depth > 0 ? max_depth : -1; J.rr_depth = rr_depth;
    J.V = V; J.product = product; J.h = h; J.seed = seed;
    J.path0 = pix_begin * spp; J.P = P;
    J.bw = bw; J.bmean = bmean; J.bcov = bcov; J.bdiff = bdiff; J.M = M; J.Kmax = Kmax;
    /* the device's rule (sdmm_scene_create: a conductor, a Phong BSDF or a
     * rough dielectric on some quad or triangle, with or without a learned
     * model, gives every compact query its own row of max(M, 2) lobes;
     * extend_learned, render_api.cpp) */
    J.lM = M;
    if (bsdf_params)
        for (int q = 0; q < n_quads + n_triangles; ++q) {
            const float kind = bsdf_params[8 * li_prim_bsdf(&S, q)];
            if ((kind == 2.0f || kind == 3.0f || kind == 4.0f) && J.lM < LI_L4_KEEP) J.lM = LI_L4_KEEP;
        }
    J.rec = rec; J.nv = nv; J.comps = comps; J.hit_bsdf = hit_bsdf;
    J.inside = inside; J.rr_eta_one = rr_eta_one; J.escaped = escaped;
    J.L = (float*)malloc(sizeof(float) * 3 * (size_t)(P > 0 ? P : 1));
    J.bounces = max_depth > 0 ? max_depth - 1 : V;
    if (nthreads < 1) nthreads = 1;
    li_range* R = (li_range*)malloc(sizeof(li_range) * (size_t)nthreads);
    pthread_t* th = (pthread_t*)malloc(sizeof(pthread_t) * (size_t)nthreads);
    const int64_t per = (P + nthreads - 1) / nthreads;
    for (int k = 0; k < nthreads; ++k) {
        R[k].J = &J;
        R[k].a = (int64_t)k * per < P ? (int64_t)k * per : P;
        R[k].b = (int64_t)(k + 1) * per < P ? (int64_t)(k + 1) * per : P;
        if (nthreads == 1) li_worker(&R[k]);
        else pthread_create(&th[k], NULL, li_worker, &R[k]);
    }
    if (nthreads > 1)
        for (int k = 0; k < nthreads; ++k) pthread_join(th[k], NULL);
    /* the film: each pixel's mean over its samples, in sample order */
    const int64_t plane = (int64_t)width * height;
    const float invs = 1.0f / (float)spp;
    for (int64_t j = 0; j < npix; ++j) {
        float acc[3] = {0.0f, 0.0f, 0.0f}, sq[3] = {0.0f, 0.0f, 0.0f};
        for (int s = 0; s < spp; ++s) {
            const float* lp = J.L + 3 * (j * spp + s);
            for (int ch = 0; ch < 3; ++ch) { acc[ch] += lp[ch]; sq[ch] += lp[ch] * lp[ch]; }
        }
        for (int ch = 0; ch < 3; ++ch) {
            image[ch * plane + pix_begin + j] = acc[ch] * invs;
            if (image_sqr) image_sqr[ch * plane + pix_begin + j] = sq[ch] * invs;
        }
    }
    free(th);
    free(R);
    free(J.L);
    free(S.quads);
    free(S.tris);
    return 0;
}
