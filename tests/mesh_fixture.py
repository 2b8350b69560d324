"""The mesh tests' shared fixture (tests/test_mesh.py, tests/test_gpu_mesh.py):
a torus 24 x 12 (576 triangles, R 1, r 0.4) plus three quads, and 4099 rays --
aimed at interior points of random triangles from a radius-3 sphere and from a
+-0.3 cube round the centre, unaimed random directions, and hand-placed rays."""
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
