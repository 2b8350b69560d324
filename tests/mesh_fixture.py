"""The mesh tests' shared fixture (tests/test_mesh.py, tests/test_gpu_mesh.py):
a torus 24 x 12 (576 triangles, R 1, r 0.4) plus three quads, and 4099 rays --
aimed at interior points of random triangles from a radius-3 sphere and from a
+-0.3 cube round the centre, unaimed random directions, and hand-placed rays.

Beside it, the harder families: spiral_mesh / deep_desc (disjoint triangles
over five or six decades of size, a BVH of exactly 24 inner levels: the
traversal stack's cap) with local and outside rays, hard_rays (grazing,
leaving the surface, -0.0 and zero components, non-finite) on the torus,
flat_grid (rays through shared vertices and edges, rays in the plane) and
tie_desc (a quad and a coplanar triangle at exactly the same distance)."""
import functools

import numpy as np

MINT = 1e-4
N_RAYS = 4099
N_AIMED_SPHERE, N_AIMED_CUBE, N_UNAIMED = 2000, 1000, 1091   # + 8 hand-placed


def base_desc(verts, tris, quads=True):
    d = {"reflectance": np.asarray([0.5, 0.5, 0.5], np.float32),
         "mesh_vertices": np.ascontiguousarray(verts, np.float32).reshape(-1),
         "triangles": np.ascontiguousarray(tris, np.int32).reshape(-1),
         "tri_bsdf": np.zeros(len(np.asarray(tris).reshape(-1, 3)), np.int32)}
    if quads:
        q = np.asarray([
            [-3.0, -0.5, -3.0, 0.0, 0.0, 6.0, 6.0, 0.0, 0.0],      # floor under the torus, normal +y
            [-3.0, -0.5, -2.0, 6.0, 0.0, 0.0, 0.0, 3.0, 0.0],      # wall behind it, normal +z
            [-0.2, 0.0, -0.2, 0.0, 0.0, 0.4, 0.4, 0.0, 0.0],       # a small quad in the hole
        ], np.float32)
        d.update(quads=q.reshape(-1), bsdf=np.zeros(3, np.int32))
    return d


def camera_fields(d, width=64, height=36):
    """A description the device scene accepts: camera and film beside the geometry."""
    return {**d, "camera_to_world": np.asarray([-1, 0, 0, 0, 0, 1, 0, 0.3, 0, 0, -1, 4.0, 0, 0, 0, 1], np.float32),
            "fov_x_deg": 40.0, "near_clip": 1e-2, "width": width, "height": height}


@functools.lru_cache(maxsize=None)
def _torus(scenes):
    return scenes.torus_mesh(24, 12, 1.0, 0.4)


def torus_desc(scenes):
    v, t = _torus(scenes)
    return base_desc(v, t)


def small_descs(scenes):
    """(name, description): a mesh of 1 triangle, of 5 (a leaf tail), and the
    torus duplicated onto itself (every hit must report the lower id)."""
    v, t = _torus(scenes)
    return [("one", base_desc(v, t[:1])), ("five", base_desc(v, t[100:105])),
            ("doubled", base_desc(v, np.concatenate([t, t])))]


@functools.lru_cache(maxsize=None)
def rays(scenes):
    """(o [4099, 3], d [4099, 3]) float32, and the index ranges by kind."""
    v, t = _torus(scenes)
    v = v.astype(np.float64)
    rng = np.random.default_rng(20240607)

    def targets(n):
        tri = t[rng.integers(0, len(t), n)]
        b = rng.uniform(0.05, 0.45, (n, 2))
        p0, p1, p2 = v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]]
        return p0 + b[:, :1] * (p1 - p0) + b[:, 1:] * (p2 - p0)

    def unit(x):
        return x / np.linalg.norm(x, axis=-1, keepdims=True)
    o1 = 3.0 * unit(rng.normal(size=(N_AIMED_SPHERE, 3)))
    d1 = unit(targets(N_AIMED_SPHERE) - o1)
    o2 = rng.uniform(-0.3, 0.3, (N_AIMED_CUBE, 3))
    d2 = unit(targets(N_AIMED_CUBE) - o2)
    o3 = np.concatenate([3.0 * unit(rng.normal(size=(N_UNAIMED // 2, 3))),
                         rng.uniform(-0.3, 0.3, (N_UNAIMED - N_UNAIMED // 2, 3))])
    d3 = unit(rng.normal(size=(N_UNAIMED, 3)))
    # hand-placed
    tri0 = t[0]
    on_tri = (v[tri0[0]] + v[tri0[1]] + v[tri0[2]]) / 3.0
    n0 = np.cross(v[tri0[1]] - v[tri0[0]], v[tri0[2]] - v[tri0[0]])
    a, b = v[tri0[0]], v[tri0[2]]                     # triangle 0's edge p0-p2: shared with triangle 1
    hand_o = np.asarray([
        [0.9, 2.0, 0.05],                             # one direction component exactly 0
        [1.0, 2.0, 0.0],                              # two
        [1.0, 0.0, 0.0],                              # inside the tube
        on_tri,                                       # on a triangle (mint 1e-4)
        0.5 * (a + b) + 2.0 * unit(n0),               # through the midpoint of a shared edge
        a - 0.5 * (b - a),                            # along that edge, in both triangles' planes
        [1.02, 2.5, 0.03],                            # a known hit (the maxt cases)
        [5.0, 5.0, 5.0],                              # misses everything
    ])
    hand_d = np.asarray([
        unit(np.asarray([0.02, -1.0, 0.0])),
        [0.0, -1.0, 0.0],
        unit(np.asarray([0.3, 0.5, 0.81])),
        unit(n0),
        -unit(n0),
        unit(b - a),
        [0.0, -1.0, 0.0],
        unit(np.asarray([1.0, 1.0, 1.0])),
    ])
    o = np.concatenate([o1, o2, o3, hand_o]).astype(np.float32)
    d = np.concatenate([d1, d2, d3, hand_d]).astype(np.float32)
    assert len(o) == N_RAYS
    n_random = N_AIMED_SPHERE + N_AIMED_CUBE + N_UNAIMED
    return o, d, {"random": slice(0, n_random), "known_hit": n_random + 6, "miss": n_random + 7}


# ---- the deep, multi-scale mesh ---------------------------------------------------
def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def spiral_mesh(n, lo, hi, seed):
    """n disjoint triangles, triangle i of size about x_i at distance x_i from
    the origin, x = geomspace(lo, hi, n) along a golden-angle spiral: (vertices
    float32 [3n, 3], triangles int32 [n, 3], x float64 [n])."""
    x = np.geomspace(lo, hi, n)
    a = 2.399963 * np.arange(n)
    centre = np.stack([x * np.cos(a), 0.2 * x * np.sin(3 * a), x * np.sin(a)], -1)
    rng = np.random.default_rng(seed)
    v = centre[:, None, :] + 0.15 * x[:, None, None] * rng.normal(size=(n, 3, 3))
    return v.reshape(-1, 3).astype(np.float32), np.arange(3 * n, dtype=np.int32).reshape(n, 3), x


# name: (n, lo, hi, seed).  The seeds are those whose BVH has exactly kBvhStack =
# 24 inner levels (deep_desc asserts it): the SAH splits of a mesh that spans
# many decades peel off a few triangles a level.
DEEP = {"wide": (2048, 1e-3, 1e3, 1), "narrow": (8192, 1e-2, 1e2, 1)}
DEEP_LEVELS = 24


@functools.lru_cache(maxsize=None)
def _spiral(which):
    return spiral_mesh(*DEEP[which])


def deep_desc(pkg, which):
    """The spiral mesh `which` of DEEP (no quads: primitive id = triangle),
    asserted at 24 inner levels."""
    v, t, _ = _spiral(which)
    d = base_desc(v, t, quads=False)
    assert pkg.mesh_bvh_dump(d)["levels"] == DEEP_LEVELS
    return d


@functools.lru_cache(maxsize=None)
def deep_rays(which, kind, n=N_RAYS, seed=77):
    """n rays aimed at interior points (barycentrics 0.05..0.45) of random
    triangles of the spiral mesh `which`.  kind "local": from p + x_i U(1, 10)
    u, x_i the target's size and u a uniform direction; "outside": from the
    sphere of radius 3 hi.  (o, d) float32 [n, 3]."""
    v, t, x = _spiral(which)
    v = v.astype(np.float64)
    rng = np.random.default_rng(seed)
    i = rng.integers(0, len(t), n)
    b = rng.uniform(0.05, 0.45, (n, 2))
    p0, p1, p2 = v[t[i, 0]], v[t[i, 1]], v[t[i, 2]]
    p = p0 + b[:, :1] * (p1 - p0) + b[:, 1:] * (p2 - p0)
    u = _unit(rng.normal(size=(n, 3)))
    if kind == "local":
        o = p + (x[i] * rng.uniform(1.0, 10.0, n))[:, None] * u
    else:
        assert kind == "outside"
        o = 3.0 * DEEP[which][2] * u
    o = o.astype(np.float32)
    return o, _unit(p - o.astype(np.float64)).astype(np.float32)


# ---- hard rays on the torus ---------------------------------------------------
N_GRAZING, N_SURFACE, N_NEGZERO = 1400, 1400, 400
# the non-finite rays and the all-zero direction: each inside a 64-lane group
# of ordinary rays (none at a group's first or last lane)
SPECIAL_AT = {"zero_dir": 70, "nan_origin": 200, "nan_dir": 330, "pinf_dir": 460, "ninf_dir": 590,
              "all_nan": 1450, "inf_origin": 2900}


@functools.lru_cache(maxsize=None)
def hard_rays(scenes):
    """(o, d, kinds) on the torus scene: grazing rays through triangle
    centroids (unit(tangent +- eps normal), eps = 10^U(-6, -2)), rays that
    start on the surface with uniform directions, rays with -0.0 direction
    components (one zero component, and two), and at SPECIAL_AT the all-zero
    direction and the non-finite rays written over ordinary ones.  kinds: the
    index ranges, "special" the sorted SPECIAL_AT indices."""
    v, t = _torus(scenes)
    v = v.astype(np.float64)
    rng = np.random.default_rng(20250311)

    def corners(n):
        tri = t[rng.integers(0, len(t), n)]
        return v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]]
    # grazing
    p0, p1, p2 = corners(N_GRAZING)
    c = (p0 + p1 + p2) / 3.0
    nrm = _unit(np.cross(p1 - p0, p2 - p0))
    phi = rng.uniform(0, 2 * np.pi, N_GRAZING)[:, None]
    e = _unit(p1 - p0)
    tangent = np.cos(phi) * e + np.sin(phi) * np.cross(nrm, e)
    eps = 10.0 ** rng.uniform(-6, -2, N_GRAZING)[:, None] * rng.choice([-1.0, 1.0], N_GRAZING)[:, None]
    dg = _unit(tangent + eps * nrm)
    og = c - rng.uniform(0.2, 3.0, N_GRAZING)[:, None] * dg
    # leaving the surface
    p0, p1, p2 = corners(N_SURFACE)
    b = rng.uniform(0.05, 0.45, (N_SURFACE, 2))
    os_ = p0 + b[:, :1] * (p1 - p0) + b[:, 1:] * (p2 - p0)
    ds = _unit(rng.normal(size=(N_SURFACE, 3)))
    # -0.0 components: from above and beside the torus
    h = N_NEGZERO // 2
    ang = rng.uniform(0, 2 * np.pi, N_NEGZERO)
    rad = rng.uniform(0.5, 1.5, N_NEGZERO)
    oz = np.stack([rad * np.cos(ang), np.full(N_NEGZERO, 2.0), rad * np.sin(ang)], -1)
    dz = np.zeros((N_NEGZERO, 3))
    dz[:, 1] = -1.0
    dz[:h, 2] = rng.uniform(-0.3, 0.3, h)                   # one zero component (x)
    dz[:h] = _unit(dz[:h])
    dz[:, 0] = -0.0
    dz[h:, 2] = np.where(np.arange(N_NEGZERO - h) % 2 == 0, -0.0, 0.0)    # two: (-0, -1, -0) and (-0, -1, +0)
    o = np.concatenate([og, os_, oz]).astype(np.float32)
    d = np.concatenate([dg, ds, dz]).astype(np.float32)
    assert np.signbit(d[-N_NEGZERO:, 0]).all() and (d[-N_NEGZERO:, 0] == 0).all()
    bad = {"zero_dir": (None, [0.0, 0.0, 0.0]), "nan_origin": ([np.nan, 0.0, 0.0], None),
           "nan_dir": (None, [0.0, np.nan, 1.0]), "pinf_dir": (None, [np.inf, -0.5, 0.1]),
           "ninf_dir": (None, [0.2, -np.inf, 0.1]), "all_nan": ([np.nan] * 3, [np.nan] * 3),
           "inf_origin": ([0.0, np.inf, 0.0], None)}
    for name, at in SPECIAL_AT.items():
        assert 0 < at % 64 < 63
        bo, bd = bad[name]
        if bo is not None:
            o[at] = bo
        if bd is not None:
            d[at] = bd
    kinds = {"grazing": slice(0, N_GRAZING), "surface": slice(N_GRAZING, N_GRAZING + N_SURFACE),
             "negzero": slice(N_GRAZING + N_SURFACE, len(o)), "special": np.asarray(sorted(SPECIAL_AT.values()))}
    return o, d, kinds


# ---- flat grid: shared vertices and edges, in-plane rays ---------------------------
def flat_grid(G=16):
    """The unit square in the plane y = 0 as 2 G^2 triangles (cell (i, j):
    triangles 2 (i G + j) and + 1, split along the diagonal): (vertices
    float32 [(G + 1)^2, 3], triangles int32 [2 G^2, 3]).  With G a power of two
    every coordinate, edge and determinant is exact in float32."""
    k = np.arange(G + 1) / G
    X, Z = np.meshgrid(k, k, indexing="ij")
    v = np.stack([X, np.zeros_like(X), Z], -1).reshape(-1, 3).astype(np.float32)
    def idx(i, j):
        return i * (G + 1) + j
    t = []
    for i in range(G):
        for j in range(G):
            t.append([idx(i, j), idx(i, j + 1), idx(i + 1, j + 1)])
            t.append([idx(i, j), idx(i + 1, j + 1), idx(i + 1, j)])
    return v, np.asarray(t, np.int32)


def flat_grid_rays(G=16):
    """(o, d, expected id) for rays (0, -1, 0) from y = 1 through every grid
    vertex and the midpoint of every edge (cell sides and diagonals): t is
    exactly 1 on every triangle that shares the point, the lowest id wins.
    The expected id is worked out exactly (the coordinates are dyadic)."""
    v, t = flat_grid(G)
    k = np.arange(G + 1) / G
    m = (np.arange(G) + 0.5) / G
    pts = [(x, z) for x in k for z in k]                    # vertices
    pts += [(x, z) for x in m for z in k]                   # edges along x
    pts += [(x, z) for x in k for z in m]                   # edges along z
    pts += [(x, z) for x in m for z in m]                   # diagonals
    pts = np.asarray(pts, np.float64)
    a, b, c = (v[t[:, k_]][:, [0, 2]].astype(np.float64) for k_ in range(3))

    def side(p, q, x):                                      # exact: products of dyadic numbers
        return (q[None, :, 0] - p[None, :, 0]) * (x[:, None, 1] - p[None, :, 1]) - \
               (q[None, :, 1] - p[None, :, 1]) * (x[:, None, 0] - p[None, :, 0])
    s0, s1, s2 = side(a, b, pts), side(b, c, pts), side(c, a, pts)
    inside = ((s0 >= 0) & (s1 >= 0) & (s2 >= 0)) | ((s0 <= 0) & (s1 <= 0) & (s2 <= 0))
    assert inside.any(1).all() and inside.sum(1).max() == 6
    expected = np.argmax(inside, 1).astype(np.int32)        # the first, so the lowest, id
    o = np.stack([pts[:, 0], np.ones(len(pts)), pts[:, 1]], -1).astype(np.float32)
    d = np.broadcast_to(np.asarray([0.0, -1.0, 0.0], np.float32), o.shape).copy()
    return o, d, expected


def flat_grid_inplane_rays(G=16):
    """Rays lying in the grid's plane: along cell sides, along a diagonal,
    through cell interiors, from outside the square and from inside it."""
    o = np.asarray([[-0.5, 0, 0.25], [-0.5, 0, 0.3], [0.25, 0, -0.5], [-0.5, 0, -0.5], [0.4, 0, 0.6],
                    [0.5, 0, 0.5], [2.0, 0, 0.5 / G], [0.3, 0, 2.0]], np.float32)
    d = np.asarray([[1, 0, 0], [1, 0, 0], [0, 0, 1], _unit(np.asarray([1.0, 0, 1.0])), _unit(np.asarray([0.3, 0, -0.7])),
                    [-0.0, 0, 1], [-1, 0, -0.0], _unit(np.asarray([0.1, 0, -1.0]))], np.float32)
    return o, d


def tie_desc():
    """One quad in y = 0 (primitive 0) under a coplanar triangle (primitive 1):
    rays (0, -1, 0) from y = 1 meet both at exactly t = 1."""
    q = np.asarray([[-1.0, 0.0, -1.0, 0.0, 0.0, 2.0, 2.0, 0.0, 0.0]], np.float32)      # p0, e1, e2: normal +y
    v = np.asarray([[-0.5, 0, -0.5], [-0.5, 0, 0.75], [0.75, 0, -0.5]], np.float32)
    return {"reflectance": np.asarray([0.5, 0.5, 0.5], np.float32), "quads": q.reshape(-1), "bsdf": np.zeros(1, np.int32),
            "mesh_vertices": v.reshape(-1), "triangles": np.asarray([0, 1, 2], np.int32), "tri_bsdf": np.zeros(1, np.int32)}


def tie_rays():
    """(o, d, expected prim): over the triangle (the quad wins the tie), over
    the quad alone, and beside both."""
    xz = np.asarray([[-0.25, -0.25], [0.0, 0.0], [-0.5, -0.5], [0.125, 0.125], [-0.375, 0.5],
                     [0.5, 0.5], [0.9, -0.9], [1.5, 0.0], [0.0, -1.25]], np.float32)
    expected = np.asarray([0, 0, 0, 0, 0, 0, 0, -1, -1], np.int32)
    o = np.stack([xz[:, 0], np.ones(len(xz), np.float32), xz[:, 1]], -1)
    d = np.broadcast_to(np.asarray([0.0, -1.0, 0.0], np.float32), o.shape).copy()
    return o, d, expected


# ---- the ladder: every stack slot a 24-level tree can use ---------------------------
# The spiral meshes are 24 levels deep, but a ray aimed at one of their
# triangles meets both children's boxes at few levels: its stack stays near
# slot 14.  The ladder is built for the walk's worst case: clusters of 6
# parallel triangles strung along +x, cluster i at x0 * ratio^i and of that
# size.  The SAH peels the far clusters off one inner node after the other, so
# a ray along +x from before the first cluster meets both children (both inner
# nodes) at every level, descends into the nearer, deeper one and pushes the
# other: slot 22 at level 23, the most a tree capped at 24 inner levels allows
# (a node of level 24 has only leaves under it).  The first cluster is 1e-8
# away, so these rays are traced with mint = 0.
LADDER = (42, 6, 2.6, 1e-8)
LADDER_MINT = 0.0


@functools.lru_cache(maxsize=None)
def ladder_mesh():
    nc, per, ratio, x0 = LADDER
    i, j = np.meshgrid(np.arange(nc), np.arange(per), indexing="ij")
    x = (x0 * ratio ** i * (1 + 0.5 * j / per)).reshape(-1)
    s = (0.3 * x0 * ratio ** i).reshape(-1)
    v = np.stack([np.stack([x, -s, -s], -1), np.stack([x, 2 * s, -s], -1), np.stack([x, -s, 2 * s], -1)], 1)
    return v.reshape(-1, 3).astype(np.float32), np.arange(3 * len(x), dtype=np.int32).reshape(-1, 3)


def ladder_desc(pkg):
    v, t = ladder_mesh()
    d = base_desc(v, t, quads=False)
    assert pkg.mesh_bvh_dump(d)["levels"] == DEEP_LEVELS
    return d


@functools.lru_cache(maxsize=None)
def ladder_rays(n=333):
    """n rays (more than a workgroup: threads t and t + 128 both hold deep
    stacks), a third each: along +x from before the first cluster, a little
    off the axis (the hit is in the first cluster, at the bottom of the
    descent: every pushed subtree is then culled); from (x0 / 2, c, c) along
    (1, 0.1, 0.1), c = 0.1 x_k of one of the 12 smallest clusters: these pass
    beside the clusters below x_k and meet a triangle further up the ladder;
    and from x_i (0.75, 0.1, 0.1) towards the axis, x_i over the ladder's
    range: they enter the tree from the side at every scale."""
    nc, per, ratio, x0 = LADDER
    rng = np.random.default_rng(99)
    na = n // 3
    nb = 2 * na
    o = np.zeros((n, 3))
    d = np.zeros((n, 3))
    o[:na, 0] = 0.5 * x0
    o[:na, 1:] = rng.uniform(-0.05 * x0, 0.05 * x0, (na, 2))
    d[:na, 0] = 1.0
    d[:na, 1:] = rng.uniform(-0.01, 0.01, (na, 2))
    c = 0.1 * x0 * ratio ** rng.uniform(0, 12, nb - na)
    o[na:nb] = np.stack([np.full(nb - na, 0.5 * x0), c, c], -1)
    d[na:nb] = np.asarray([1.0, 0.1, 0.1])
    xi = x0 * ratio ** rng.uniform(0, nc, n - nb)
    o[nb:] = xi[:, None] * np.asarray([0.75, 0.1, 0.1])
    d[nb:] = rng.normal(size=(n - nb, 3)) * 0.2 + np.asarray([1.0, -0.1, -0.1])
    return o.astype(np.float32), _unit(d).astype(np.float32)
