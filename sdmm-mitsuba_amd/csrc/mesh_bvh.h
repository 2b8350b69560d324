// mesh_bvh.h -- the triangle mesh of a scene: a binary BVH in a flat array and
// its traversal (host + device, one source), built on the host by
// mesh_bvh.cpp.  No HIP include.
//
// Node (64 B, one cache line): both children's boxes, so one fetch decides
// both descents.  child[c] >= 0: an inner node; < 0: a leaf, ~child = first *
// 8 + count (count <= 4) into the leaf-ordered triangle array.  Boxes are float,
// widened outward by one ulp per bound: a triangle lying in an axis plane has a
// box the slab test cannot reject.
//
// Traversal: one ray per caller, nearer child first, the farther one pushed.
// A leaf child is tested at once (nothing pushed), so the stack holds at most
// one entry per inner level above the deepest: kBvhStack entries serve
// kBvhStack + 1 inner levels; the builder caps the inner levels at kBvhStack,
// so the deepest slot a walk writes is kBvhStack - 2 (the tests' ladder mesh
// reaches it; the last slot is spare).  The stack is the caller's: the kernels keep it in LDS as [level][thread]
// (a runtime-indexed private array would go to scratch), the host in an array.
#pragma once
#include "mesh_intersect.h"
#include "shading_normal.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace sdmm {

constexpr int kBvhStack = 24;       // stack entries = the cap on inner levels
constexpr int kBvhLeaf = 4;         // triangles per leaf
constexpr int kMeshMaxTriangles = 1 << 26;   // median splits of that many fit the cap (24 levels)

struct alignas(64) BvhNode {
    float lo[2][3], hi[2][3];
    int32_t child[2];
    int32_t pad[2];
};
static_assert(sizeof(BvhNode) == 64, "BvhNode layout");

// Slab test of one child box against t in [mint, tb].  *tn: the entry distance
// (ordering).  A direction component of 0 is decided by the origin alone (no 0
// * inf), so a ray lying in a face of the box is inside.  The distances the
// triangle test returns are not exact: the rounding of its cross and dot
// products scales with |o - p0| |e1| |e2| / |det|, not with t (2.5e-5 relative
// on the test rays, origins 3 units away; more at grazing incidence).  The
// walk must visit every triangle whose COMPUTED t could win or tie, or it
// would differ from the brute-force loop, so the interval is widened by 1e-4
// relative to its larger end.  That is not a derived bound: BVH == loop bitwise
// is tested, not proven for every input.  The envelope it is tested on
// (tests/test_mesh.py on the host, tests/test_gpu_mesh.py on the device):
//   - the 24 x 12 torus with aimed and random rays from 3 units away, grazing
//     rays tilted 1e-6..1e-2 out of a triangle's plane, rays that start on
//     the surface (mint 1e-4 and 1e-3), direction components of +-0, the zero
//     direction and non-finite rays (these hit nothing);
//   - a flat grid met through its vertices and edges and by rays in its plane;
//   - disjoint triangles of size x at distance x, x over 1e-3..1e3 and
//     1e-2..1e2 (24 inner levels), seen from 1..10 sizes away and, the second,
//     from 300 units away: a distance of up to 2e5 triangle sizes;
//   - a ladder of clusters over 1e-8..1e9 whose axial rays fill the stack.
// Seen from 3000 units the 1e-3..1e3 mesh (up to 2e7 sizes away) is the edge:
// past about 1e6 sizes Moeller-Trumbore's cancellation makes the loop report
// hits on triangles the ray passes several widths beside, which the walk
// never visits; test_scale_envelope allows a difference only there.  With the
// margin at 0 the walk still equals the loop on every family above, and
// differs on 63 of those 20 000 far rays.  No cull at equality.
SDMM_MESH_HD bool bvh_box(const float lo[3], const float hi[3], const float o[3], const float d[3],
                          const float inv[3], float mint, float tb, float* tn) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    float n = -__builtin_inff(), f = __builtin_inff();
    for (int a = 0; a < 3; ++a) {
        float an, af;
        if (d[a] == 0.0f) {
            const bool in = o[a] >= lo[a] && o[a] <= hi[a];
            an = in ? -__builtin_inff() : __builtin_inff();
            af = __builtin_inff();
        } else {
            const float t0 = (lo[a] - o[a]) * inv[a], t1 = (hi[a] - o[a]) * inv[a];
            an = t0 < t1 ? t0 : t1;
            af = t0 < t1 ? t1 : t0;
        }
        n = an > n ? an : n;
        f = af < f ? af : f;
    }
    *tn = n;
    const float an_ = __builtin_fabsf(n), af_ = __builtin_fabsf(f);
    const float s = 1e-4f * (an_ > af_ ? an_ : af_);
    const float nw = n - s, fw = f + s;
    return nw <= fw && fw >= mint && nw <= tb;
}

// Closest hit over the whole mesh through the BVH (tri_consider's rule).
// Stack: push(level, node), pop(level).
template <class Stack>
SDMM_MESH_HD void bvh_closest(const BvhNode* nodes, const MeshTri* tris, int id_off, const float o[3],
                              const float d[3], float mint, float maxt, int& best, float& tb, Stack& st) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float inv[3] = {1.0f / d[0], 1.0f / d[1], 1.0f / d[2]};
    int node = 0, sp = 0;
    for (;;) {
        const BvhNode N = nodes[node];
        float tn[2];
        bool hit[2];
        for (int c = 0; c < 2; ++c) hit[c] = bvh_box(N.lo[c], N.hi[c], o, d, inv, mint, tb, &tn[c]);
        // leaves at once
        for (int c = 0; c < 2; ++c)
            if (hit[c] && N.child[c] < 0) {
                const int v = ~N.child[c], first = v >> 3, cnt = v & 7;
                for (int i = 0; i < cnt; ++i) tri_consider(tris[first + i], id_off, o, d, mint, maxt, best, tb);
                hit[c] = false;
            }
        // (a leaf may have shortened tb: the inner children are weighed again)
        for (int c = 0; c < 2; ++c)
            if (hit[c]) hit[c] = bvh_box(N.lo[c], N.hi[c], o, d, inv, mint, tb, &tn[c]);
        if (hit[0] && hit[1]) {
            const int nearer = tn[1] < tn[0] ? 1 : 0;
            st.push(sp++, N.child[1 - nearer]);
            node = N.child[nearer];
        } else if (hit[0] || hit[1]) {
            node = N.child[hit[0] ? 0 : 1];
        } else {
            if (sp == 0) return;
            node = st.pop(--sp);
        }
    }
}

// The same by a loop over every triangle (mode 1: the check of the BVH)
SDMM_MESH_HD void mesh_brute(const MeshTri* tris, int n, int id_off, const float o[3], const float d[3], float mint,
                             float maxt, int& best, float& tb) {
    for (int i = 0; i < n; ++i) tri_consider(tris[i], id_off, o, d, mint, maxt, best, tb);
}

}  // namespace sdmm

// ---- host: build ----
#include <string>
#include <vector>

namespace sdmm {

struct MeshInput {
    int n_vertices = 0;
    const float* vertices = nullptr;        // 3 per vertex, world
    int n_triangles = 0;
    const int32_t* triangles = nullptr;     // 3 vertex indices each
    const int32_t* bsdf = nullptr;          // per triangle
    const int32_t* emitter = nullptr;       // nullable, -1: none
    const int32_t* flip = nullptr;          // nullable
    const float* normals = nullptr;         // nullable: 3 per vertex, world, used as given
    int n_bsdfs = 0, n_emitters = 0;
};

struct MeshBvh {
    std::vector<MeshTri> tris;      // leaf order
    std::vector<MeshHit> hits;      // caller's order
    std::vector<MeshShade> shade;   // caller's order; empty without vertex normals
    std::vector<BvhNode> nodes;     // nodes[0]: the root
    int levels = 0;                 // inner levels (root = 1)
    float mn[3], mx[3];             // AABB of all the vertices
};

// Validates and builds (deterministic, single-threaded).  max_levels: the cap
// on inner levels (0: kBvhStack).  false: *err says why.
bool mesh_build(const MeshInput& in, int max_levels, MeshBvh* out, std::string* err);

// Closest hit on the host for one ray: mode 0 the BVH, 1 the loop
void mesh_closest_host(const MeshBvh& m, int id_off, int mode, const float o[3], const float d[3], float mint,
                       float maxt, int& best, float& tb);

}  // namespace sdmm
