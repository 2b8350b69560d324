"""The shading-normal tests' shared cases (tests/test_shading_cases.py on the
host, tests/test_gpu_shading_normals.py on the device) and a numpy float32
restatement of the hit-normal rule, written from the normals part of
fillIntersectionRecord (mitsuba/include/mitsuba/render/skdtree.h:355-396) and
from Triangle::rayIntersect (core/triangle.h:109-145) for the barycentrics:

    b  = (1 - u - v, u, v)
    ns = (n0 b.x + n1 b.y + n2 b.z) / |.|, negated where the triangle is flipped
    ng = the winding's face normal, negated when dot(ng, ns) < 0
    a sum of length 0 or a non-finite one: ns = ng = the face normal (flipped)
    quads, and a mesh without vertex normals: ns = ng = the face normal (flipped)

Every operation is one float32 numpy operation, in the library's order, so the
library's entries are expected to agree bitwise."""
import functools

import numpy as np

import mesh_fixture as mf

F = np.float32


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], -1)


def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def _unit_face(e1, e2, flip):
    n = _cross(e1, e2)
    ln = np.sqrt(_dot(n, n))
    sg = np.where(flip != 0, F(-1.0), F(1.0)).astype(F)
    return sg[:, None] * n / ln[:, None]


def restate(desc, o, d, prim):
    """(ns, ng) float32 [nq, 3] of the hits `prim` (the closest-hit search's
    answer, -1: a miss -> zeros) of rays o, d on a description."""
    o = np.ascontiguousarray(o, F).reshape(-1, 3)
    d = np.ascontiguousarray(d, F).reshape(-1, 3)
    prim = np.asarray(prim)
    nq = len(o)
    ns = np.zeros((nq, 3), F)
    ng = np.zeros((nq, 3), F)
    n_quads = 0
    if "quads" in desc and np.asarray(desc["quads"]).size:
        q = np.asarray(desc["quads"], F).reshape(-1, 3, 3)
        n_quads = len(q)
        fl = np.asarray(desc.get("flip_normals", np.zeros(n_quads, np.int32)))
        qn = _unit_face(q[:, 1], q[:, 2], fl)
        on = (prim >= 0) & (prim < n_quads)
        ns[on] = ng[on] = qn[prim[on]]
    if "triangles" not in desc:
        return ns, ng
    V = np.asarray(desc["mesh_vertices"], F).reshape(-1, 3)
    T = np.asarray(desc["triangles"], np.int64).reshape(-1, 3)
    flip_all = np.asarray(desc["tri_flip_normals"]) if desc.get("tri_flip_normals") is not None \
        else np.zeros(len(T), np.int32)
    on = np.nonzero(prim >= n_quads)[0]
    if not len(on):
        return ns, ng
    ti = prim[on] - n_quads
    tri, flip = T[ti], flip_all[ti]
    p0 = V[tri[:, 0]]
    e1, e2 = V[tri[:, 1]] - p0, V[tri[:, 2]] - p0
    face = _unit_face(e1, e2, flip)
    ns[on] = ng[on] = face
    if desc.get("mesh_normals") is None:
        return ns, ng
    N = np.asarray(desc["mesh_normals"], F).reshape(-1, 3)
    oo, dd = o[on], d[on]
    with np.errstate(all="ignore"):
        # Triangle::rayIntersect's u, v
        pvec = _cross(dd, e2)
        det = _dot(e1, pvec)
        inv_det = F(1.0) / det
        tvec = oo - p0
        u = _dot(tvec, pvec) * inv_det
        qvec = _cross(tvec, e1)
        v = _dot(dd, qvec) * inv_det
        b0 = F(1.0) - u - v
        n0, n1, n2 = N[tri[:, 0]], N[tri[:, 1]], N[tri[:, 2]]
        s = n0 * b0[:, None] + n1 * u[:, None] + n2 * v[:, None]
        ln = np.sqrt(_dot(s, s))
        ok = (ln > 0) & np.isfinite(ln)
        sg = np.where(flip != 0, F(-1.0), F(1.0)).astype(F)
        sn = sg[:, None] * (s / ln[:, None])
        g = sg[:, None] * face                                   # the flip undone: the winding's normal
        g = np.where((_dot(g, sn) < 0)[:, None], -g, g)
    out_ns, out_ng = face.copy(), face.copy()
    out_ns[ok], out_ng[ok] = sn[ok], g[ok]
    ns[on], ng[on] = out_ns, out_ng
    return ns, ng


# ---- the cases -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _torus(scenes):
    return scenes.torus_mesh(24, 12, 1.0, 0.4, normals=True)


def torus_desc(scenes, **changes):
    """mesh_fixture's torus 24 x 12 with its three quads, carrying the
    analytic vertex normals."""
    v, t, n = _torus(scenes)
    d = mf.base_desc(v, t)
    d["mesh_normals"] = n.reshape(-1).copy()
    d.update(changes)
    return d


def vanish_desc():
    """Two triangles in y = 0 with dyadic corners and opposing vertex normals
    (0, +-1, 0): on the line u = 1/2 the interpolated sum is exactly 0 -- the
    fallback; triangle 1 is flipped.  No quads: primitive id = triangle."""
    v = np.asarray([[0, 0, 0], [1, 0, 0], [0, 0, 1], [2, 0, 0], [3, 0, 0], [2, 0, 1]], F)
    n = np.asarray([[0, 1, 0], [0, -1, 0], [0, 1, 0]] * 2, F)
    return {"reflectance": np.asarray([0.5, 0.5, 0.5], F), "mesh_vertices": v.reshape(-1),
            "triangles": np.arange(6, dtype=np.int32), "tri_bsdf": np.zeros(2, np.int32),
            "tri_flip_normals": np.asarray([0, 1], np.int32), "mesh_normals": n.reshape(-1)}


def vanish_rays():
    """(o, d, vanishing): rays (0, -1, 0) from y = 1; the first four meet the
    triangles where u = 1/2 exactly (v = 1/4 and 1/8: every product exact)."""
    xz = np.asarray([[0.5, 0.25], [0.5, 0.125], [2.5, 0.25], [2.5, 0.125],
                     [0.25, 0.25], [0.125, 0.5], [2.25, 0.25], [2.75, 0.125], [1.5, 0.25]], F)
    o = np.stack([xz[:, 0], np.ones(len(xz), F), xz[:, 1]], -1)
    d = np.broadcast_to(np.asarray([0.0, -1.0, 0.0], F), o.shape).copy()
    return o, d, np.arange(len(xz)) < 4


def cases(scenes):
    """name -> (description, o, d): the torus under mesh_fixture's benign and
    hard ray families (hits on triangles and quads, misses, non-finite rays),
    vertex normals that disagree with the winding (ng is turned), flipped
    triangles, and the vanishing sum."""
    ob, db, _ = mf.rays(scenes)
    oh, dh, _ = mf.hard_rays(scenes)
    v, t, n = _torus(scenes)
    flip = (np.arange(len(t)) % 3 == 0).astype(np.int32)
    ov, dv, _ = vanish_rays()
    return {
        "torus_benign": (torus_desc(scenes), ob, db),
        "torus_hard": (torus_desc(scenes), oh, dh),
        "disagree": (torus_desc(scenes, mesh_normals=(-n).reshape(-1).copy()), ob, db),
        "flip": (torus_desc(scenes, tri_flip_normals=flip), ob, db),
        "unnormalised": (torus_desc(scenes, mesh_normals=(n * (1.0 + np.arange(len(n))[:, None] % 5)).astype(F).reshape(-1)),
                         ob, db),
        "vanish": (vanish_desc(), ov, dv),
    }
