// mesh_bvh.cpp -- host build of the triangle BVH (mesh_bvh.h): validation,
// binned SAH over the triangle centroids (16 bins an axis) with a median split
// where SAH does not separate, leaves of at most 4 triangles in contiguous
// ranges, inner levels capped at the traversal stack's capacity.  Plain C++,
// deterministic, single-threaded; no HIP.
#include "mesh_bvh.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace sdmm {
namespace {

constexpr int kBins = 16;

struct Box {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    void add(const float p[3]) {
        for (int a = 0; a < 3; ++a) {
            lo[a] = std::min(lo[a], p[a]);
            hi[a] = std::max(hi[a], p[a]);
        }
    }
    void add(const Box& b) {
        for (int a = 0; a < 3; ++a) {
            lo[a] = std::min(lo[a], b.lo[a]);
            hi[a] = std::max(hi[a], b.hi[a]);
        }
    }
    double area() const {
        const double x = (double)hi[0] - lo[0], y = (double)hi[1] - lo[1], z = (double)hi[2] - lo[2];
        return x < 0.0 ? 0.0 : 2.0 * (x * y + y * z + z * x);
    }
};

struct Prim {
    Box box;
    float c[3];     // centroid of the box
    int32_t id;
};

// inner levels a median-split tree over n triangles needs
int median_levels(int64_t n) {
    int l = 0;
    while (n > kBvhLeaf) {
        n = (n + 1) / 2;
        ++l;
    }
    return l;
}

struct Builder {
    std::vector<Prim> prims;
    std::vector<BvhNode> nodes;
    int cap = kBvhStack, levels = 0;
    bool too_deep = false;

    static int32_t leaf_ref(int first, int count) { return ~(int32_t)(first * 8 + count); }

    Box range_box(int b, int e) const {
        Box r;
        for (int i = b; i < e; ++i) r.add(prims[(size_t)i].box);
        return r;
    }

    // the split position of [b, e) (b < mid < e); level: this inner node's
    int split(int b, int e, int level) {
        const int n = e - b;
        Box cb;
        for (int i = b; i < e; ++i) cb.add(prims[(size_t)i].c);
        int best_axis = -1, best_bin = -1;
        double best_cost = INFINITY;
        for (int a = 0; a < 3; ++a) {
            const float ext = cb.hi[a] - cb.lo[a];
            if (!(ext > 0.0f)) continue;
            Box bb[kBins];
            int cnt[kBins] = {0};
            const float scale = (float)kBins / ext;
            for (int i = b; i < e; ++i) {
                const Prim& p = prims[(size_t)i];
                const int k = std::min(kBins - 1, std::max(0, (int)((p.c[a] - cb.lo[a]) * scale)));
                bb[k].add(p.box);
                ++cnt[k];
            }
            double right_area[kBins];
            int right_cnt[kBins];
            Box acc;
            int c = 0;
            for (int k = kBins - 1; k > 0; --k) {
                acc.add(bb[k]);
                c += cnt[k];
                right_area[k] = acc.area();
                right_cnt[k] = c;
            }
            Box left;
            int lc = 0;
            for (int k = 0; k < kBins - 1; ++k) {
                left.add(bb[k]);
                lc += cnt[k];
                if (lc == 0 || right_cnt[k + 1] == 0) continue;
                const double cost = left.area() * lc + right_area[k + 1] * right_cnt[k + 1];
                if (cost < best_cost) {
                    best_cost = cost;
                    best_axis = a;
                    best_bin = k;
                }
            }
        }
        int mid = -1;
        if (best_axis >= 0) {
            const int a = best_axis;
            const float scale = (float)kBins / (cb.hi[a] - cb.lo[a]);
            const float lo = cb.lo[a];
            auto it = std::stable_partition(prims.begin() + b, prims.begin() + e, [&](const Prim& p) {
                const int k = std::min(kBins - 1, std::max(0, (int)((p.c[a] - lo) * scale)));
                return k <= best_bin;
            });
            mid = (int)(it - prims.begin());
            // the SAH split must leave room under the cap for both sides
            const int deeper = median_levels(std::max(mid - b, e - mid));
            if (mid <= b || mid >= e || level + deeper > cap) mid = -1;
        }
        if (mid < 0) {
            // median split: along the widest centroid axis, ties by id (a total order)
            int a = 0;
            for (int k = 1; k < 3; ++k)
                if (cb.hi[k] - cb.lo[k] > cb.hi[a] - cb.lo[a]) a = k;
            std::sort(prims.begin() + b, prims.begin() + e, [a](const Prim& x, const Prim& y) {
                return x.c[a] < y.c[a] || (x.c[a] == y.c[a] && x.id < y.id);
            });
            mid = b + (n + 1) / 2;
        }
        return mid;
    }

    // builds the inner node over [b, e) (more than a leaf's worth) at `level`
    int32_t build(int b, int e, int level) {
        if (level + median_levels((e - b + 1) / 2) > cap) {
            too_deep = true;
            return 0;
        }
        levels = std::max(levels, level);
        const int32_t me = (int32_t)nodes.size();
        nodes.emplace_back();
        const int mid = split(b, e, level);
        const int rb[2] = {b, mid}, re[2] = {mid, e};
        for (int c = 0; c < 2; ++c) {
            const Box bx = range_box(rb[c], re[c]);
            const int32_t ref = re[c] - rb[c] <= kBvhLeaf ? leaf_ref(rb[c], re[c] - rb[c]) : build(rb[c], re[c], level + 1);
            if (too_deep) return 0;
            BvhNode& N = nodes[(size_t)me];
            for (int a = 0; a < 3; ++a) {
                N.lo[c][a] = std::nextafter(bx.lo[a], -INFINITY);
                N.hi[c][a] = std::nextafter(bx.hi[a], INFINITY);
            }
            N.child[c] = ref;
        }
        return me;
    }
};

}  // namespace

bool mesh_build(const MeshInput& in, int max_levels, MeshBvh* out, std::string* err) {
    auto fail = [&](const char* m) {
        if (err) *err = m;
        return false;
    };
    if (in.n_triangles < 1 || in.n_triangles > kMeshMaxTriangles || in.n_vertices < 1 || !in.vertices ||
        !in.triangles)
        return fail("mesh: vertices and triangles needed (at most 2^26 triangles)");
    if (!in.bsdf) return fail("mesh: tri_bsdf is required with triangles");
    const int cap = max_levels > 0 ? std::min(max_levels, kBvhStack) : kBvhStack;
    for (int a = 0; a < 3; ++a) {
        out->mn[a] = INFINITY;
        out->mx[a] = -INFINITY;
    }
    for (int64_t i = 0; i < (int64_t)in.n_vertices; ++i)
        for (int a = 0; a < 3; ++a) {
            const float x = in.vertices[3 * i + a];
            if (!std::isfinite(x)) return fail("mesh: non-finite vertex");
            out->mn[a] = std::min(out->mn[a], x);
            out->mx[a] = std::max(out->mx[a], x);
        }
    if (in.normals)
        for (int64_t i = 0; i < (int64_t)in.n_vertices; ++i) {
            const float* n = in.normals + 3 * i;
            if (!std::isfinite(n[0]) || !std::isfinite(n[1]) || !std::isfinite(n[2]))
                return fail("mesh: non-finite vertex normal");
            if (n[0] == 0.0f && n[1] == 0.0f && n[2] == 0.0f) return fail("mesh: vertex normal of length 0");
        }
    const int nt = in.n_triangles;
    Builder B;
    B.cap = cap;
    B.prims.resize((size_t)nt);
    out->hits.resize((size_t)nt);
    out->shade.resize(in.normals ? (size_t)nt : 0);
    std::vector<MeshTri> prepared((size_t)nt);
    for (int i = 0; i < nt; ++i) {
        const int32_t* ix = in.triangles + 3 * (int64_t)i;
        for (int k = 0; k < 3; ++k)
            if (ix[k] < 0 || ix[k] >= in.n_vertices) return fail("mesh: vertex index out of range");
        const float* p0 = in.vertices + 3 * (int64_t)ix[0];
        const float* p1 = in.vertices + 3 * (int64_t)ix[1];
        const float* p2 = in.vertices + 3 * (int64_t)ix[2];
        MeshTri& T = prepared[(size_t)i];
        for (int a = 0; a < 3; ++a) {
            T.p0[a] = p0[a];
            T.e1[a] = p1[a] - p0[a];
            T.e2[a] = p2[a] - p0[a];
        }
        T.id = i;
        const float n[3] = {T.e1[1] * T.e2[2] - T.e1[2] * T.e2[1], T.e1[2] * T.e2[0] - T.e1[0] * T.e2[2],
                            T.e1[0] * T.e2[1] - T.e1[1] * T.e2[0]};
        const float len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        if (!(len > 0.0f) || !std::isfinite(len)) return fail("mesh: zero-area triangle");
        MeshHit& H = out->hits[(size_t)i];
        const float sg = (in.flip && in.flip[i]) ? -1.0f : 1.0f;
        for (int a = 0; a < 3; ++a) H.n[a] = sg * n[a] / len;
        H.bsdf = in.bsdf[i];
        H.emitter = in.emitter ? in.emitter[i] : -1;
        if (H.bsdf < 0 || H.bsdf >= in.n_bsdfs || H.emitter < -1 || (H.emitter >= 0 && H.emitter >= in.n_emitters))
            return fail("mesh: material index out of range");
        if (in.normals) {
            MeshShade& V = out->shade[(size_t)i];
            V.tri = T;
            for (int a = 0; a < 3; ++a) {
                V.n0[a] = in.normals[3 * (int64_t)ix[0] + a];
                V.n1[a] = in.normals[3 * (int64_t)ix[1] + a];
                V.n2[a] = in.normals[3 * (int64_t)ix[2] + a];
            }
            V.flip = (in.flip && in.flip[i]) ? 1 : 0;
        }
        Prim& P = B.prims[(size_t)i];
        P.box.add(p0);
        P.box.add(p1);
        P.box.add(p2);
        for (int a = 0; a < 3; ++a) P.c[a] = 0.5f * P.box.lo[a] + 0.5f * P.box.hi[a];
        P.id = i;
    }
    if (nt <= kBvhLeaf) {
        // one leaf under a root whose second child is empty (an inverted box, no triangles)
        B.nodes.emplace_back();
        BvhNode& N = B.nodes[0];
        const Box bx = B.range_box(0, nt);
        for (int a = 0; a < 3; ++a) {
            N.lo[0][a] = std::nextafter(bx.lo[a], -INFINITY);
            N.hi[0][a] = std::nextafter(bx.hi[a], INFINITY);
            N.lo[1][a] = INFINITY;
            N.hi[1][a] = -INFINITY;
        }
        N.child[0] = Builder::leaf_ref(0, nt);
        N.child[1] = Builder::leaf_ref(0, 0);
        B.levels = 1;
    } else {
        B.build(0, nt, 1);
        if (B.too_deep) return fail("mesh: the BVH would be deeper than the traversal stack");
    }
    out->tris.resize((size_t)nt);
    for (int i = 0; i < nt; ++i) out->tris[(size_t)i] = prepared[(size_t)B.prims[(size_t)i].id];
    out->nodes = std::move(B.nodes);
    out->levels = B.levels;
    return true;
}

namespace {
struct HostStack {
    int32_t v[kBvhStack];
    void push(int level, int32_t node) { v[level] = node; }
    int32_t pop(int level) const { return v[level]; }
};
}  // namespace

void mesh_closest_host(const MeshBvh& m, int id_off, int mode, const float o[3], const float d[3], float mint,
                       float maxt, int& best, float& tb) {
    if (mode == 0) {
        HostStack st;
        bvh_closest(m.nodes.data(), m.tris.data(), id_off, o, d, mint, maxt, best, tb, st);
    } else {
        mesh_brute(m.tris.data(), (int)m.tris.size(), id_off, o, d, mint, maxt, best, tb);
    }
}

}  // namespace sdmm
