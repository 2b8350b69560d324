// mesh_intersect.h -- the ray / triangle test of the mesh path, host + device,
// float: Triangle::rayIntersect (mitsuba/include/mitsuba/core/triangle.h:
// 109-145) restated -- Moeller-Trumbore with det == 0 rejected, inv_det = 1 /
// det, the u, v, u + v range checks, then t.  Contraction is off: the host
// entries and the kernels are meant to agree bitwise.  No HIP include; under
// hipcc the functions are __host__ __device__.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SDMM_MESH_HD __host__ __device__ __forceinline__
#else
#define SDMM_MESH_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace sdmm {

// A triangle prepared for the test (40 B): corner and the two edges; id: its
// index in the caller's triangle list (the BVH reorders the array)
struct MeshTri {
    float p0[3], e1[3], e2[3];
    int32_t id;
};
static_assert(sizeof(MeshTri) == 40, "MeshTri layout");

// What only a confirmed hit reads (20 B), indexed by the caller's triangle
// index: the unit face normal normalize((p1 - p0) x (p2 - p0)) (flip applied),
// BSDF and emitter (-1: none)
struct MeshHit {
    float n[3];
    int32_t bsdf, emitter;
};
static_assert(sizeof(MeshHit) == 20, "MeshHit layout");

// true: the ray o + t d meets the triangle at *t (any sign); *u, *v: the
// test's own barycentrics of the hit, p = (1 - u - v) p0 + u p1 + v p2
SDMM_MESH_HD bool tri_intersect_uv(const MeshTri& T, const float o[3], const float d[3], float* t, float* u_out,
                                   float* v_out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float pvec[3] = {d[1] * T.e2[2] - d[2] * T.e2[1], d[2] * T.e2[0] - d[0] * T.e2[2],
                           d[0] * T.e2[1] - d[1] * T.e2[0]};
    const float det = T.e1[0] * pvec[0] + T.e1[1] * pvec[1] + T.e1[2] * pvec[2];
    if (det == 0.0f) return false;
    const float inv_det = 1.0f / det;
    const float tvec[3] = {o[0] - T.p0[0], o[1] - T.p0[1], o[2] - T.p0[2]};
    const float u = (tvec[0] * pvec[0] + tvec[1] * pvec[1] + tvec[2] * pvec[2]) * inv_det;
    if (u < 0.0f || u > 1.0f) return false;
    const float qvec[3] = {tvec[1] * T.e1[2] - tvec[2] * T.e1[1], tvec[2] * T.e1[0] - tvec[0] * T.e1[2],
                           tvec[0] * T.e1[1] - tvec[1] * T.e1[0]};
    const float v = (d[0] * qvec[0] + d[1] * qvec[1] + d[2] * qvec[2]) * inv_det;
    // (inverted comparison: catches NaNs)
    if (v >= 0.0f && u + v <= 1.0f) {
        *t = (T.e2[0] * qvec[0] + T.e2[1] * qvec[1] + T.e2[2] * qvec[2]) * inv_det;
        *u_out = u;
        *v_out = v;
        return true;
    }
    return false;
}
// (the closest-hit search does not keep the barycentrics: shading_normal.h
// runs the test again on the winner alone)
SDMM_MESH_HD bool tri_intersect(const MeshTri& T, const float o[3], const float d[3], float* t) {
    float u, v;
    return tri_intersect_uv(T, o, d, t, &u, &v);
}

// The closest-hit rule for a triangle (every path goes through here): t in
// (mint, maxt), the smallest t wins, on exactly equal t the lowest primitive
// id.  best / tb: the running winner (primitive id, -1: none, tb = maxt then)
// and its distance; id_off: the triangle ids' offset (n_quads).
SDMM_MESH_HD void tri_consider(const MeshTri& T, int id_off, const float o[3], const float d[3], float mint,
                               float maxt, int& best, float& tb) {
    float t;
    if (!tri_intersect(T, o, d, &t)) return;
    if (!(t > mint && t < maxt)) return;
    const int id = id_off + T.id;
    if (t < tb || (t == tb && id < best)) {
        tb = t;
        best = id;
    }
}

}  // namespace sdmm
