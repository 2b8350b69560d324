"""The texture tests' shared cases (tests/test_texture_cases.py on the host,
tests/test_gpu_texture.py on the device) and a numpy float32 restatement of
csrc/texture.h, written from the reference's sources:

    its.uv     a quad: the parametric coordinates (a, b) of the hit (shapes/
               rectangle.cpp:163, p0 as the local (-1, -1) corner); a triangle:
               t0 b.x + t1 b.y + t2 b.z with b = (1 - u - v, u, v), or (u, v)
               without texture coordinates (render/skdtree.h:399-405), u, v
               from Triangle::rayIntersect (core/triangle.h:109-145)
    the lookup Texture2D::eval: uv * uvScale + uvOffset (librender/texture.cpp:
               112-121), then BitmapTexture::eval(uv) (textures/bitmap.cpp:
               431-454): MIPMap::evalBilinear, or evalBox with the nearest
               filter, over evalTexel's boundary rules (render/mipmap.h:503-596)
    departures a non-finite uv gives 0 in both filters; a texel coordinate
               whose floor does not fit int32 gives 0

Every operation is one float32 numpy operation, in the library's order, so the
library's entries are expected to agree bitwise."""
import functools
import itertools

import numpy as np

F = np.float32
FILTERS = (0, 1)                       # bilinear, nearest
WRAPS = (0, 1, 2, 3, 4)                # repeat, clamp, mirror, zero, one
SCALES = (1.0, 7.5, -2.0)
OFFSET = (0.375, -1.25)                # dyadic, non-zero


def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], -1)


# ---- the lookup -------------------------------------------------------------------------
def _wrap(x, n, mode):
    """evalTexel's boundary rule on one axis: (index int64, fill float32 or NaN
    where the index holds)."""
    x = x.astype(np.int64)
    inside = (x >= 0) & (x < n)
    fill = np.full(len(x), np.nan, F)
    if mode == 0:
        idx = np.mod(x, n)
    elif mode == 1:
        idx = np.clip(x, 0, n - 1)
    elif mode == 2:
        r = np.mod(x, 2 * n)
        idx = np.where(r >= n, 2 * n - r - 1, r)
    else:
        idx = np.where(inside, x, 0)
        fill[~inside] = F(0.0) if mode == 3 else F(1.0)
    return np.where(inside, x, idx), fill


def _texel(tex, x, y):
    px = np.asarray(tex["pixels"], F)
    h, w = px.shape[:2]
    xi, fx = _wrap(x, w, int(tex["wrap_u"]))
    yi, fy = _wrap(y, h, int(tex["wrap_v"]))
    out = px[yi, xi]
    fill = np.where(np.isnan(fx), fy, fx)          # the u axis decides first
    return np.where(np.isnan(fill)[:, None], out, fill[:, None]).astype(F)


def _floor_int(x):
    f = np.floor(x)
    ok = (f >= F(-2147483648.0)) & (f < F(2147483648.0))
    return np.where(ok, f, F(0)).astype(np.int64), f, ok


def tex_eval(tex, uv):
    """tex_eval of csrc/texture.h: tex a dict as the description's (integer
    filter / wrap codes, uv_scale / uv_offset pairs), uv float32 [n, 2] ->
    float32 [n, 3]."""
    uv = np.asarray(uv, F).reshape(-1, 2)
    px = np.asarray(tex["pixels"], F)
    h, w = px.shape[:2]
    sc = np.broadcast_to(np.asarray(tex.get("uv_scale", 1.0), F), (2,))
    of = np.broadcast_to(np.asarray(tex.get("uv_offset", 0.0), F), (2,))
    out = np.zeros((len(uv), 3), F)
    with np.errstate(all="ignore"):
        uvx = uv[:, 0] * sc[0] + of[0]
        uvy = uv[:, 1] * sc[1] + of[1]
        fin = np.isfinite(uvx) & np.isfinite(uvy)
        if int(tex.get("filter", 0)) == 1:
            x, _, okx = _floor_int(uvx * F(w))
            y, _, oky = _floor_int(uvy * F(h))
            ok = fin & okx & oky
            out[ok] = _texel(tex, x, y)[ok]
            return out
        u = uvx * F(w) - F(0.5)
        v = uvy * F(h) - F(0.5)
        x, fx, okx = _floor_int(u)
        y, fy, oky = _floor_int(v)
        ok = fin & okx & oky
        dx1 = u - fx
        dx2 = F(1.0) - dx1
        dy1 = v - fy
        dy2 = F(1.0) - dy1
        t00, t01 = _texel(tex, x, y), _texel(tex, x, y + 1)
        t10, t11 = _texel(tex, x + 1, y), _texel(tex, x + 1, y + 1)
        val = t00 * dx2[:, None] * dy2[:, None] + t01 * dx2[:, None] * dy1[:, None] \
            + t10 * dx1[:, None] * dy2[:, None] + t11 * dx1[:, None] * dy1[:, None]
    out[ok] = val[ok]
    return out


# ---- the hit's uv -----------------------------------------------------------------------
def hit_uv(desc, o, d, prim):
    """its.uv float32 [nq, 2] of the hits `prim` (the search's answer; a miss:
    zeros) of rays o, d on a description."""
    o = np.ascontiguousarray(o, F).reshape(-1, 3)
    d = np.ascontiguousarray(d, F).reshape(-1, 3)
    prim = np.asarray(prim)
    uv = np.zeros((len(o), 2), F)
    n_quads = 0
    with np.errstate(all="ignore"):
        if "quads" in desc and np.asarray(desc["quads"]).size:
            q = np.asarray(desc["quads"], F).reshape(-1, 3, 3)
            n_quads = len(q)
            on = np.nonzero((prim >= 0) & (prim < n_quads))[0]
            if len(on):
                p0, e1, e2 = (q[prim[on], k] for k in range(3))
                fl = np.asarray(desc.get("flip_normals", np.zeros(n_quads, np.int32)))[prim[on]]
                n = _cross(e1, e2)
                ln = np.sqrt(_dot(n, n))
                sg = np.where(fl != 0, F(-1.0), F(1.0)).astype(F)
                qn = sg[:, None] * n / ln[:, None]
                a1, a2 = _cross(e2, n), _cross(n, e1)
                g1, g2 = a1 / _dot(e1, a1)[:, None], a2 / _dot(e2, a2)[:, None]
                oo, dd = o[on], d[on]
                denom = _dot(dd, qn)
                t = _dot(p0 - oo, qn) / denom
                r = oo + t[:, None] * dd - p0
                uv[on] = np.stack([_dot(r, g1), _dot(r, g2)], -1)
        on = np.nonzero(prim >= n_quads)[0]
        if len(on):
            V = np.asarray(desc["mesh_vertices"], F).reshape(-1, 3)
            T = np.asarray(desc["triangles"], np.int64).reshape(-1, 3)
            tri = T[prim[on] - n_quads]
            p0 = V[tri[:, 0]]
            e1, e2 = V[tri[:, 1]] - p0, V[tri[:, 2]] - p0
            oo, dd = o[on], d[on]
            pvec = _cross(dd, e2)
            inv_det = F(1.0) / _dot(e1, pvec)
            tvec = oo - p0
            u = _dot(tvec, pvec) * inv_det
            v = _dot(dd, _cross(tvec, e1)) * inv_det
            if desc.get("mesh_uvs") is None:
                uv[on] = np.stack([u, v], -1)
            else:
                tc = np.asarray(desc["mesh_uvs"], F).reshape(-1, 2)
                b0 = F(1.0) - u - v
                uv[on] = tc[tri[:, 0]] * b0[:, None] + tc[tri[:, 1]] * u[:, None] + tc[tri[:, 2]] * v[:, None]
    return uv


def _codes(tex):
    from_name = {"bilinear": 0, "nearest": 1, "repeat": 0, "clamp": 1, "mirror": 2, "zero": 3, "one": 4}
    return {**tex, **{k: (from_name[tex[k]] if isinstance(tex.get(k), str) else int(tex.get(k, 0)))
                      for k in ("filter", "wrap_u", "wrap_v")}}


def restate(desc, o, d, prim):
    """(uv [nq, 2], rgb [nq, 3]) float32 of the hits `prim`: its.uv and the
    effective reflectance -- the hit BSDF's texture there, or its row; zeros on
    a miss."""
    prim = np.asarray(prim)
    uv = hit_uv(desc, o, d, prim)
    n_quads = np.asarray(desc["quads"]).size // 9 if "quads" in desc else 0
    bsdf = np.full(len(prim), -1, np.int64)
    onq = (prim >= 0) & (prim < n_quads)
    if onq.any():
        bsdf[onq] = np.asarray(desc["bsdf"])[prim[onq]]
    ont = prim >= n_quads
    if ont.any():
        bsdf[ont] = np.asarray(desc["tri_bsdf"])[prim[ont] - n_quads]
    refl = np.asarray(desc["reflectance"], F).reshape(-1, 3)
    rgb = np.zeros((len(prim), 3), F)
    hit = prim >= 0
    rgb[hit] = refl[bsdf[hit]]
    if desc.get("bsdf_texture") is not None:
        bt = np.asarray(desc["bsdf_texture"])
        for ti in np.unique(bt[bt >= 0]):
            on = hit & (bt[np.maximum(bsdf, 0)] == ti)
            if on.any():
                rgb[on] = tex_eval(_codes(desc["textures"][int(ti)]), uv[on])
    return uv, rgb


# ---- the cases --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pixels(w, h):
    """w x h texels of distinct, non-dyadic colours in (0.05, 0.95)."""
    rng = np.random.default_rng(1000 * w + h)
    return rng.uniform(0.05, 0.95, (h, w, 3)).astype(F)


SIZES = ((1, 1), (2, 2), (3, 5), (4, 4))   # (w, h)


@functools.lru_cache(maxsize=None)
def configs():
    """Every texture of the sweep: sizes x filters x the 25 wrap pairs x scales
    (with the non-zero offset): 600 dicts."""
    out = []
    for (w, h), f, wu, wv, s in itertools.product(SIZES, FILTERS, WRAPS, WRAPS, SCALES):
        out.append({"pixels": pixels(w, h), "filter": f, "wrap_u": wu, "wrap_v": wv,
                    "uv_scale": (s, s), "uv_offset": OFFSET})
    return out


def cell_points():
    """(x, z) float32 [n, 2] in the unit square: the 9 x 9 grid of eighths
    (corners, edges, the texel centres and edges of a 2 x 2 and a 4 x 4 bitmap,
    a two-triangle square's vertices, sides and diagonal) and 19 others."""
    k = np.arange(9) / 8.0
    grid = np.stack(np.meshgrid(k, k, indexing="ij"), -1).reshape(-1, 2)
    rng = np.random.default_rng(5)
    return np.concatenate([grid, rng.uniform(0.0, 1.0, (19, 2))]).astype(F)


GEOMETRIES = ("quad", "mesh_uv", "mesh_bary", "mesh_flip")
# the two-triangle square's texture coordinates: below 0 and above 1, dyadic
SQUARE_UVS = np.asarray([[-0.5, -0.25], [1.5, 0.0], [1.5, 2.0], [-0.5, 1.75]], F)


def sweep(geometry, texs=None, spacing=2.0):
    """(description, o, d): one unit square in the plane y = 0 per texture, the
    k-th at x in [2 k, 2 k + 1] with BSDF k carrying texture k, under rays (0,
    -1, 0) from y = 1 through cell_points() of every square (all coordinates
    dyadic or exact).  geometry: "quad" -- a parallelogram; "mesh_uv" -- two
    triangles with SQUARE_UVS; "mesh_bary" -- the same without texture
    coordinates; "mesh_flip" -- with them and the first triangle flipped."""
    texs = configs() if texs is None else texs
    n = len(texs)
    x0 = (spacing * np.arange(n)).astype(F)
    desc = {"reflectance": np.tile(np.asarray([0.5, 0.25, 0.125], F), n),
            "textures": list(texs), "bsdf_texture": np.arange(n, dtype=np.int32)}
    if geometry == "quad":
        q = np.zeros((n, 3, 3), F)
        q[:, 0, 0] = x0
        q[:, 1, 0] = 1.0          # e1 = +x: a
        q[:, 2, 2] = 1.0          # e2 = +z: b
        desc.update(quads=q.reshape(-1), bsdf=np.arange(n, dtype=np.int32))
    else:
        corner = np.asarray([[0, 0, 0], [1, 0, 0], [1, 0, 1], [0, 0, 1]], F)
        v = corner[None] + np.stack([x0, np.zeros(n, F), np.zeros(n, F)], -1)[:, None]
        t = (4 * np.arange(n)[:, None, None] + np.asarray([[0, 1, 2], [0, 2, 3]])[None]).astype(np.int32)
        desc.update(mesh_vertices=v.reshape(-1), triangles=t.reshape(-1),
                    tri_bsdf=np.repeat(np.arange(n, dtype=np.int32), 2))
        if geometry != "mesh_bary":
            desc["mesh_uvs"] = np.tile(SQUARE_UVS, (n, 1)).reshape(-1)
        if geometry == "mesh_flip":
            desc["tri_flip_normals"] = np.tile(np.asarray([1, 0], np.int32), n)
    pts = cell_points()
    o = np.zeros((n, len(pts), 3), F)
    o[:, :, 0] = x0[:, None] + pts[None, :, 0]
    o[:, :, 1] = 1.0
    o[:, :, 2] = pts[None, :, 1]
    o = o.reshape(-1, 3)
    d = np.broadcast_to(np.asarray([0.0, -1.0, 0.0], F), o.shape).copy()
    return desc, o, d


# texture coordinates only a mesh can carry: huge (the texel coordinate leaves
# int32, or the scaled uv overflows to inf), negative zero
PROBE_UVS = np.asarray([[1e9, 0.5], [0.5, -1e9], [3e38, 0.5], [0.5, -3e38], [-0.0, -0.0], [2.0 ** 29, 0.25],
                        [-(2.0 ** 29), 0.25], [0.25, 2.0 ** 31], [1.0, 1.0], [0.0, 0.0]], F)


def probe(texs=None):
    """(description, o, d): per texture and per PROBE_UVS entry one triangle
    whose three vertices all carry that uv, met through its vertex p1 (u = 1:
    the interpolated uv is the entry itself) and at an inner point."""
    texs = [c for c in configs() if np.asarray(c["pixels"]).shape[:2] == (5, 3)] if texs is None else texs
    n, m = len(texs), len(PROBE_UVS)
    k = np.arange(n * m)
    x0 = (2.0 * k).astype(F)
    corner = np.asarray([[0, 0, 0], [1, 0, 0], [0, 0, 1]], F)
    v = corner[None] + np.stack([x0, np.zeros(len(k), F), np.zeros(len(k), F)], -1)[:, None]
    desc = {"reflectance": np.tile(np.asarray([0.5, 0.25, 0.125], F), n), "textures": list(texs),
            "bsdf_texture": np.arange(n, dtype=np.int32), "mesh_vertices": v.reshape(-1),
            "triangles": np.arange(3 * len(k), dtype=np.int32), "tri_bsdf": (k // m).astype(np.int32),
            "mesh_uvs": np.repeat(np.tile(PROBE_UVS, (n, 1)), 3, axis=0).reshape(-1)}
    at = np.asarray([[1.0, 0.0], [0.25, 0.5]], F)
    o = np.zeros((len(k), 2, 3), F)
    o[:, :, 0] = x0[:, None] + at[None, :, 0]
    o[:, :, 1] = 1.0
    o[:, :, 2] = at[None, :, 1]
    o = o.reshape(-1, 3)
    d = np.broadcast_to(np.asarray([0.0, -1.0, 0.0], F), o.shape).copy()
    return desc, o, d


def edge_uvs():
    """uv float32 [n, 2] for tex_eval directly (tests/cpp/texture_check.cpp):
    0 and 1 exactly, texel centres and edges, negative, above 1, -0.0, NaN and
    +-inf, and texel coordinates past int32."""
    one = [0.0, -0.0, 1.0, 0.125, 0.25, 0.375, 0.5, 0.1, 0.3, 0.7, 0.9, -0.25, -0.3, -1.0, -1.7, 1.25, 2.0, 2.6,
           -7.5, 17.0, 1e9, -1e9, 2.0 ** 29, -(2.0 ** 29), 2.0 ** 31, 3e38, -3e38, np.nan, np.inf, -np.inf]
    a = np.asarray(list(itertools.product(one, [0.0, 0.3, 1.0, -0.6, 1.4])) +
                   list(itertools.product([0.3, 0.5], one)), F)
    return a


def camera_fields(d, width=32, height=18, origin=(0.5, 2.0, 0.5)):
    """A description the device scene accepts: a camera above the first unit
    square looking straight down (x grows along the image's rows, z down the image)."""
    cam = np.asarray([-1, 0, 0, origin[0], 0, 0, -1, origin[1], 0, -1, 0, origin[2], 0, 0, 0, 1], F)
    return {**d, "camera_to_world": cam, "fov_x_deg": 40.0, "near_clip": 1e-2, "width": width, "height": height}
