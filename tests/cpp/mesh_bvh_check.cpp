// mesh_bvh_check.cpp -- the BVH build and both traversal modes (mesh_bvh.h /
// mesh_bvh.cpp) as a stand-alone program for a sanitizer build (tests/
// test_mesh.py): the fixture files of the Python tests (the torus, and meshes
// whose trees are as deep as the stack allows), then 20 000 random triangles
// over repeated vertices with 10 000 rays.  Every ray's (prim, t) must agree
// bitwise between the BVH and the loop, and with a walk over a stack that
// checks its bounds and reports the deepest slot written.  Writes each
// fixture's hits to <fixture>.out (prim[n] int32, t[n] float32).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "mesh_bvh.h"

using namespace sdmm;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}
static float uni() { return (float)(rnd() & 0xFFFFFF) * (1.0f / 16777216.0f); }

// kBvhStack entries like the host's and the kernels' stacks, every access checked
struct CheckedStack {
    int32_t v[kBvhStack];
    int deepest = -1;
    bool out_of_bounds = false;
    void push(int level, int32_t node) {
        if (level < 0 || level >= kBvhStack) {
            out_of_bounds = true;
            return;
        }
        v[level] = node;
        if (level > deepest) deepest = level;
    }
    int32_t pop(int level) {
        if (level < 0 || level > deepest) {
            out_of_bounds = true;
            return 0;
        }
        return v[level];
    }
};

static int run(const std::vector<float>& v, const std::vector<int32_t>& tri, const std::vector<float>& o,
               const std::vector<float>& d, float mint, std::vector<int32_t>* prim_out, std::vector<float>* t_out) {
    const int nt = (int)(tri.size() / 3);
    std::vector<int32_t> bsdf((size_t)nt, 0);
    MeshInput in;
    in.n_vertices = (int)(v.size() / 3);
    in.vertices = v.data();
    in.n_triangles = nt;
    in.triangles = tri.data();
    in.bsdf = bsdf.data();
    in.n_bsdfs = 1;
    MeshBvh m;
    std::string err;
    if (!mesh_build(in, 0, &m, &err)) {
        std::printf("build failed: %s\n", err.c_str());
        return 1;
    }
    if (m.levels < 1 || m.levels > kBvhStack || (int)m.tris.size() != nt) {
        std::printf("bad tree: %d levels, %zu triangles\n", m.levels, m.tris.size());
        return 1;
    }
    const size_t nq = o.size() / 3;
    int hits = 0;
    CheckedStack cs;
    for (size_t i = 0; i < nq; ++i) {
        int best[3] = {-1, -1, -1};
        float tb[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
        for (int mode = 0; mode < 2; ++mode)
            mesh_closest_host(m, 0, mode, &o[3 * i], &d[3 * i], mint, __builtin_inff(), best[mode], tb[mode]);
        bvh_closest(m.nodes.data(), m.tris.data(), 0, &o[3 * i], &d[3 * i], mint, __builtin_inff(), best[2], tb[2], cs);
        if (cs.out_of_bounds) {
            std::printf("ray %zu: the walk left the stack's %d entries\n", i, kBvhStack);
            return 1;
        }
        if (best[0] != best[1] || std::memcmp(&tb[0], &tb[1], sizeof(float)) != 0 || best[0] != best[2] ||
            std::memcmp(&tb[0], &tb[2], sizeof(float)) != 0) {
            std::printf("ray %zu: BVH (%d, %.9g) != loop (%d, %.9g) or != the checked walk (%d, %.9g)\n", i, best[0],
                        tb[0], best[1], tb[1], best[2], tb[2]);
            return 1;
        }
        hits += best[0] >= 0;
        if (prim_out) {
            prim_out->push_back(best[0]);
            t_out->push_back(tb[0]);
        }
    }
    std::printf("%d triangles, %d levels, %zu nodes, %zu rays, %d hits, deepest stack slot %d\n", nt, m.levels,
                m.nodes.size(), nq, hits, cs.deepest);
    return 0;
}

// one fixture file: int32 nv, nt, nq; float mint; vertices, triangles, origins, directions
static int run_file(const char* path) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) return 2;
    int32_t hdr[3];
    float mint;
    if (std::fread(hdr, sizeof(int32_t), 3, f) != 3 || std::fread(&mint, sizeof(float), 1, f) != 1) return 2;
    std::vector<float> v((size_t)hdr[0] * 3), o((size_t)hdr[2] * 3), d((size_t)hdr[2] * 3);
    std::vector<int32_t> tri((size_t)hdr[1] * 3);
    if (std::fread(v.data(), sizeof(float), v.size(), f) != v.size() ||
        std::fread(tri.data(), sizeof(int32_t), tri.size(), f) != tri.size() ||
        std::fread(o.data(), sizeof(float), o.size(), f) != o.size() ||
        std::fread(d.data(), sizeof(float), d.size(), f) != d.size())
        return 2;
    std::fclose(f);
    std::vector<int32_t> prim;
    std::vector<float> t;
    if (run(v, tri, o, d, mint, &prim, &t)) return 1;
    std::FILE* g = std::fopen((std::string(path) + ".out").c_str(), "wb");
    if (!g) return 2;
    std::fwrite(prim.data(), sizeof(int32_t), prim.size(), g);
    std::fwrite(t.data(), sizeof(float), t.size(), g);
    std::fclose(g);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::printf("usage: mesh_bvh_check <fixture file>...\n");
        return 2;
    }
    for (int k = 1; k < argc; ++k)
        if (const int rc = run_file(argv[k])) return rc;

    // 20 000 random triangles over 3 000 vertices on a coarse grid (repeated
    // positions: coincident centroids, coplanar and duplicated triangles)
    const int NV = 3000, NT = 20000, NQ = 10000;
    std::vector<float> rv((size_t)NV * 3);
    for (float& x : rv) x = (float)(rnd() % 33) * 0.125f - 2.0f;
    std::vector<int32_t> rt;
    while ((int)rt.size() < 3 * NT) {
        const int a = (int)(rnd() % NV), b = (int)(rnd() % NV), c = (int)(rnd() % NV);
        const float* p0 = &rv[3 * a];
        const float* p1 = &rv[3 * b];
        const float* p2 = &rv[3 * c];
        const float e1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
        const float e2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
        const float n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        if (n[0] == 0.0f && n[1] == 0.0f && n[2] == 0.0f) continue;   // (zero area is refused by the build)
        // short edges only, so that the tree has something to separate
        if (e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2] > 1.0f || e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2] > 1.0f)
            continue;
        rt.push_back(a);
        rt.push_back(b);
        rt.push_back(c);
        if (rnd() % 16 == 0 && (int)rt.size() < 3 * NT) {   // the same triangle again
            rt.push_back(a);
            rt.push_back(b);
            rt.push_back(c);
        }
    }
    std::vector<float> ro((size_t)NQ * 3), rd((size_t)NQ * 3);
    for (int i = 0; i < NQ; ++i) {
        for (int a = 0; a < 3; ++a) {
            ro[3 * i + a] = uni() * 6.0f - 3.0f;
            rd[3 * i + a] = uni() * 2.0f - 1.0f;
        }
        if (i % 50 == 0) rd[3 * i + (i / 50) % 3] = 0.0f;                 // axis-parallel components
        if (i % 125 == 0) ro[3 * i] = (float)(rnd() % 33) * 0.125f - 2.0f;   // origins on the vertex grid's planes
    }
    if (run(rv, rt, ro, rd, 1e-4f, nullptr, nullptr)) return 1;
    std::printf("mesh_bvh_check ok\n");
    return 0;
}
