// shading_normal.h -- the shading and geometric normal of a hit on a triangle
// with vertex normals, host + device, float: the normals part of
// fillIntersectionRecord (mitsuba/include/mitsuba/render/skdtree.h:355-396)
// restated.  Contraction is off: the host entry (sdmm_scene_shading_host), the
// device entry (sdmm_scene_shading) and the Li kernels all call
// shading_normals and are meant to agree bitwise.  No HIP include; under hipcc
// the functions are __host__ __device__.
//
// The closest-hit search keeps only (primitive, t), so the triangle test runs
// once more on the winner: the same source on the same operands, hence the
// same u, v the search saw.
#pragma once
#include "mesh_intersect.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace sdmm {

// What a hit on a mesh with vertex normals reads (80 B), indexed by the
// caller's triangle index: the triangle as the test takes it (tri.id: that
// index), its three vertex normals as given (not normalised, skdtree.h:384-388)
// and the triangle's flip flag
struct MeshShade {
    MeshTri tri;
    float n0[3], n1[3], n2[3];
    int32_t flip;
};
static_assert(sizeof(MeshShade) == 80, "MeshShade layout");

// ns, ng of the hit of the ray (o, d) on triangle V; face: MeshHit::n, the
// unit face normal with the flip applied.
//   b  = (1 - u - v, u, v)
//   ns = (n0 b.x + n1 b.y + n2 b.z) / |.|, negated where flipped (trimesh.cpp:
//        624-628 negates the vertex normals; the winding is left alone)
//   ng = the winding's face normal (face without the flip), negated when
//        dot(ng, ns) < 0 (skdtree.h:390-396)
// The sum is divided by its length (Mitsuba multiplies by the reciprocal):
// a sum along a coordinate axis gives exactly the unit vector, so exact
// axis-aligned vertex normals change nothing.  A sum of length 0 or a
// non-finite one (Mitsuba would carry a NaN), or a ray the test rejects:
// ns = ng = face.
SDMM_MESH_HD void shading_normals(const MeshShade& V, const float face[3], const float o[3], const float d[3],
                                  float ns[3], float ng[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    for (int a = 0; a < 3; ++a) ns[a] = ng[a] = face[a];
    float t, u, v;
    if (!tri_intersect_uv(V.tri, o, d, &t, &u, &v)) return;
    const float b0 = 1.0f - u - v;
    float s[3];
    for (int a = 0; a < 3; ++a) s[a] = V.n0[a] * b0 + V.n1[a] * u + V.n2[a] * v;
    const float len = __builtin_sqrtf(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
    // (inverted comparison: catches NaNs)
    if (!(len > 0.0f) || len == __builtin_inff()) return;
    const float sg = V.flip ? -1.0f : 1.0f;
    for (int a = 0; a < 3; ++a) {
        ns[a] = sg * (s[a] / len);
        ng[a] = sg * face[a];           // the winding's normal: the flip undone
    }
    if (ng[0] * ns[0] + ng[1] * ns[1] + ng[2] * ns[2] < 0.0f)
        for (int a = 0; a < 3; ++a) ng[a] = -ng[a];
}

// The same from the test's outcome (hit; u, v), for a caller that ran the test
// itself because it needs the barycentrics for the hit's uv as well
// (texture.h): the test on the winner then runs once for both.  (Stated twice
// rather than called from shading_normals: the kernels that call that one keep
// their code.)
SDMM_MESH_HD void shading_normals_at(const MeshShade& V, const float face[3], bool hit, float u, float v,
                                     float ns[3], float ng[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    for (int a = 0; a < 3; ++a) ns[a] = ng[a] = face[a];
    if (!hit) return;
    const float b0 = 1.0f - u - v;
    float s[3];
    for (int a = 0; a < 3; ++a) s[a] = V.n0[a] * b0 + V.n1[a] * u + V.n2[a] * v;
    const float len = __builtin_sqrtf(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
    if (!(len > 0.0f) || len == __builtin_inff()) return;
    const float sg = V.flip ? -1.0f : 1.0f;
    for (int a = 0; a < 3; ++a) {
        ns[a] = sg * (s[a] / len);
        ng[a] = sg * face[a];
    }
    if (ng[0] * ns[0] + ng[1] * ns[1] + ng[2] * ns[2] < 0.0f)
        for (int a = 0; a < 3; ++a) ng[a] = -ng[a];
}

}  // namespace sdmm
