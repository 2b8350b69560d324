"""Triangle meshes in the device Li: Scene.intersect (BVH and brute force)
against intersect_host bitwise, the scene AABB, a quad-only description
unchanged by the new fields, a convex diffuse body in a furnace (exactly rho),
the Cornell box with its cubes as triangles against the quad scene, and the
torus scene (guided, product, brute-force A/B in a child process); the same
bitwise equality on meshes of 24 inner levels, on a ladder whose rays fill the
LDS stack, on hard rays (grazing, surface-leaving, signed zeros, non-finite),
on shared vertices and edges, on exact ties and on small batches, and the Li
kernels' own stack on a 24-level tree against the loop."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import mesh_fixture as mf  # noqa: E402
from test_gpu_li import _check_producer, _train, _tree  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


def _planes(a, gpu):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a[:, i])).to(gpu) for i in range(3)]


def _bits(prim, t):
    return prim.cpu().numpy(), t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("which", ["torus", "one", "five", "doubled"])
def test_scene_intersect_equals_host_bitwise(pkg, scenes, gpu, which):
    """4099 rays (the last workgroup has a tail): device BVH == device brute
    force == intersect_host on (prim, t)."""
    desc = mf.torus_desc(scenes) if which == "torus" else dict(mf.small_descs(scenes))[which]
    o, d, _ = mf.rays(scenes)
    sc = pkg.Scene(mf.camera_fields(desc))
    op, dp = _planes(o, gpu), _planes(d, gpu)
    hp, ht = pkg.intersect_host(desc, o, d, mf.MINT, np.inf, 0)
    assert (hp >= 3).any() and (hp < 0).any()
    for mode in (0, 1):
        prim, t = _bits(*sc.intersect(op, dp, mf.MINT, float("inf"), mode))
        assert np.array_equal(prim, hp), (which, mode)
        assert np.array_equal(t, ht.view(np.uint32)), (which, mode)
    if which == "doubled":
        assert hp.max() < 3 + 576


def test_normalization_includes_the_mesh(pkg, scenes, gpu):
    v, t = scenes.torus_mesh(24, 12, 1.0, 0.4, to_world=np.array([[1.0, 0, 0, 2.5], [0, 1.0, 0, 0.25], [0, 0, 2.0, -4]]))
    desc = mf.base_desc(v, t)
    smin, snorm, tmin, tmax = pkg.Scene(mf.camera_fields(desc)).normalization()
    q = desc["quads"].reshape(-1, 3, 3)
    corners = np.concatenate([q[:, 0], q[:, 0] + q[:, 1], q[:, 0] + q[:, 2], q[:, 0] + q[:, 1] + q[:, 2], v])
    lo, hi = corners.min(0), corners.max(0)
    assert hi[0] > 3.0 and lo[2] < -3.0                   # the mesh reaches beyond the quads
    assert np.array_equal(smin, lo)
    ext = (hi - lo).astype(np.float32)
    assert np.float32(snorm) == ext.max()
    assert np.array_equal(tmax, ext / ext.max() + np.float32(1e-5))


def test_quad_only_description_renders_the_same(pkg, scenes, gpu):
    """n_triangles = 0 (the other mesh fields set): bitwise the image of the
    description without the new fields, guided and unguided."""
    import torch
    plain = scenes.cornell_box(64, 36)
    v, _ = scenes.convex_mesh()
    with_fields = {**plain, "mesh_vertices": v.reshape(-1), "triangles": np.zeros(0, np.int32),
                   "tri_bsdf": np.zeros(4, np.int32), "tri_emitter": np.zeros(4, np.int32),
                   "tri_flip_normals": np.ones(4, np.int32)}
    a, b = pkg.Scene(plain), pkg.Scene(with_fields)
    assert b.n_triangles == 0 and b.n_quads == a.n_quads
    tree = _tree(pkg, a)
    node_mix = _train(pkg, a, tree, 4, 8, K=16)
    assert any(m is not None for m in node_mix)
    for guided in (False, True):
        ia, _, sa = a.render(tree, node_mix if guided else None, spp=4, guided=guided, seed=31)
        ia = ia.clone()
        ib, _, sb = b.render(tree, node_mix if guided else None, spp=4, guided=guided, seed=31)
        assert torch.equal(ia, ib) and sa == sb
        assert not guided or sa["guided_queries"] > 0


# ---- convex furnace ------------------------------------------------------------
RHO = 0.6


def _convex_furnace(scenes, flip=False):
    """The box [-3, 3]^3 of unit emitters of tests/test_gpu_roughdielectric.py
    with convex_mesh() (diffuse, rho 0.6) at its centre; the camera at (0, 0,
    2.5) with a 20 degree field of view: every pixel sees the mesh."""
    cube = np.array([[3.0, 0, 0, 0], [0, 3.0, 0, 0], [0, 0, 3.0, 0]])
    quads = [np.concatenate(f) for f in scenes._cube_faces(cube)]
    v, t = scenes.convex_mesh()
    cam = np.asarray([-1, 0, 0, 0, 0, 1, 0, 0, 0, 0, -1, 2.5, 0, 0, 0, 1], np.float32)
    return {"quads": np.asarray(quads, np.float32).reshape(-1), "flip_normals": np.ones(6, np.int32),
            "bsdf": np.zeros(6, np.int32), "reflectance": np.asarray([0, 0, 0, RHO, RHO, RHO], np.float32),
            "emitter": np.zeros(6, np.int32), "radiance": np.ones(3, np.float32), "camera_to_world": cam,
            "fov_x_deg": 20.0, "near_clip": 1e-2, "width": 64, "height": 36,
            "mesh_vertices": v.reshape(-1), "triangles": t.reshape(-1), "tri_bsdf": np.ones(len(t), np.int32),
            "tri_flip_normals": np.full(len(t), int(flip), np.int32)}


def _mean_vs_rho(img, what, plog):
    px = img.cpu().numpy().astype(np.float64)
    assert np.isfinite(px).all()
    px = px.mean(0)
    se = float(px.std(ddof=1) / np.sqrt(px.size))
    # (BSDF-only samples are all exactly rho: se is 0 then, and what is left
    # is the film's float32 sum of 256 equal terms, below 256 * 2^-24 relative)
    slack = 256 * 2.0 ** -24 * RHO
    s = abs(px.mean() - RHO) / max(se, 1e-300)
    print(f"convex furnace {what}: mean {px.mean():.7f} +- {se:.2e} (rho {RHO})")
    plog(f"mesh_furnace_{what}_abs_err", abs(px.mean() - RHO), 4 * se + slack, mean=float(px.mean()), se=se)
    assert abs(px.mean() - RHO) <= 4 * se + slack, (what, px.mean(), se, s)


def test_convex_furnace(pkg, scenes, gpu, plog):
    """A convex diffuse body in a uniform furnace returns exactly rho: a
    self-hit after the 1e-4 ray offset or a wrong winding lowers the mean."""
    desc = _convex_furnace(scenes)
    sc = pkg.Scene(desc)
    # every pixel sees the mesh
    o, d = _camera_rays(desc)
    prim, _ = sc.intersect(_planes(o, gpu), _planes(d, gpu), 1e-2, float("inf"), 0)
    assert int(prim.min()) >= 6
    tree = _tree(pkg, sc)
    img, _, st = sc.render(tree, None, spp=256, guided=False, seed=2101)
    _mean_vs_rho(img, "bsdf", plog)
    assert st["segments"] == st["paths"]                  # one bounce each: no ray meets the body again
    flipped = pkg.Scene(_convex_furnace(scenes, flip=True))
    img0 = flipped.render(tree, None, spp=16, guided=False, seed=2102)[0]
    assert float(img0.abs().max()) == 0.0
    node_mix = _train(pkg, sc, tree, 4, 8, K=16)
    img, _, st = sc.render(tree, node_mix, spp=256, guided=True, seed=2103)
    assert st["guided_queries"] > 0
    _mean_vs_rho(img, "guided", plog)


def _triangle_furnace(scenes, body=True, flip_box=False):
    """The same furnace with no quad at all: the box's six unit emitters as
    twelve inward-facing triangles (tri_emitter 0, the quads' emitter array
    absent), the convex body (tri_emitter -1) inside it."""
    cube = np.array([[3.0, 0, 0, 0], [0, 3.0, 0, 0], [0, 0, 3.0, 0]])
    inward = [np.concatenate((p0, e2, e1)) for p0, e1, e2 in scenes._cube_faces(cube)]
    v, t = scenes.quads_to_triangles(np.asarray(inward, np.float32))
    bsdf, emitter, flip = [0] * len(t), [0] * len(t), [int(flip_box)] * len(t)
    if body:
        bv, bt = scenes.convex_mesh()
        t = np.concatenate([t, bt + len(v)])
        v = np.concatenate([v, bv])
        bsdf += [1] * len(bt); emitter += [-1] * len(bt); flip += [0] * len(bt)
    d = _convex_furnace(scenes)
    for k in ("quads", "flip_normals", "bsdf", "emitter"):
        del d[k]
    d.update(mesh_vertices=v.reshape(-1), triangles=t.reshape(-1), tri_bsdf=np.asarray(bsdf, np.int32),
             tri_emitter=np.asarray(emitter, np.int32), tri_flip_normals=np.asarray(flip, np.int32))
    return d


def test_emissive_triangles_without_quads(pkg, scenes, gpu, plog):
    """Emitters on triangles only (n_quads = 0, no quad emitter array): the
    radiance table is there for them.  The body in the triangle furnace
    returns rho as in the quad furnace; without the body every camera ray sees
    an emitter's front (the image is the radiance, 1); with the box's normals
    flipped the emitters face outward and the image is 0."""
    desc = _triangle_furnace(scenes)
    sc = pkg.Scene(desc)
    assert sc.n_quads == 0 and sc.n_triangles == 12 + 32
    tree = _tree(pkg, sc)
    img, _, st = sc.render(tree, None, spp=256, guided=False, seed=2201)
    _mean_vs_rho(img, "triangle_emitters_bsdf", plog)
    assert st["segments"] <= st["paths"]
    empty = pkg.Scene(_triangle_furnace(scenes, body=False))
    seen = empty.render(tree, None, spp=4, guided=False, seed=2202)[0]
    assert float(seen.min()) == 1.0 and float(seen.max()) == 1.0
    outward = pkg.Scene(_triangle_furnace(scenes, flip_box=True))
    assert float(outward.render(tree, None, spp=16, guided=False, seed=2203)[0].abs().max()) == 0.0
    # the host and device closest hits agree on this mesh-only scene as well
    o, d = _camera_rays(desc)
    hp, ht = pkg.intersect_host(desc, o, d, 1e-2, np.inf, 0)
    prim, t = _bits(*sc.intersect(_planes(o, gpu), _planes(d, gpu), 1e-2, float("inf"), 0))
    assert np.array_equal(prim, hp) and np.array_equal(t, ht.view(np.uint32)) and hp.min() >= 12


# ---- Cornell box, cubes as triangles -------------------------------------------
def _camera_rays(desc, float64=False):
    """The camera kernel's rays through the pixel centres (numpy)."""
    W, H = desc["width"], desc["height"]
    cam = desc["camera_to_world"].astype(np.float64).reshape(4, 4)[:3]
    tanx = np.tan(0.5 * np.radians(desc["fov_x_deg"]))
    SX, SY = np.meshgrid((np.arange(W) + 0.5) / W, (np.arange(H) + 0.5) / H)
    l = np.stack([(1 - 2 * SX) * tanx, (1 - 2 * SY) * tanx / (W / H), np.ones_like(SX)], -1).reshape(-1, 3)
    d = l @ cam[:, :3].T
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = np.broadcast_to(cam[:, 3], d.shape)
    if float64:
        return o.copy(), d
    return np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)


def _edge_distance64(desc, o, d, diagonal_of):
    """Per ray: the distance (scene units) of its float64 closest quad hit to
    that quad's edges, and for the quads listed in diagonal_of to the
    diagonal p0 -> p0 + e1 + e2 (the two triangles' shared edge)."""
    q = desc["quads"].reshape(-1, 3, 3).astype(np.float64)
    n = np.cross(q[:, 1], q[:, 2])
    den = d @ n.T
    with np.errstate(all="ignore"):
        t = ((q[None, :, 0] - o[:, None]) * n[None]).sum(-1) / den
        r = o[:, None] + t[..., None] * d[:, None] - q[None, :, 0]
        l1, l2 = np.linalg.norm(q[:, 1], axis=-1), np.linalg.norm(q[:, 2], axis=-1)
        # (the Cornell box's quads are rectangles: coordinates along the edges)
        x, y = (r * (q[:, 1] / l1[:, None])[None]).sum(-1), (r * (q[:, 2] / l2[:, None])[None]).sum(-1)
        ok = (den != 0) & (t > 1e-2) & (x >= 0) & (x <= l1) & (y >= 0) & (y <= l2)
        t = np.where(ok, t, np.inf)
    win = np.argmin(t, 1)
    rows = np.arange(len(o))
    xw, yw, a, b = x[rows, win], y[rows, win], l1[win], l2[win]
    dist = np.minimum(np.minimum(xw, a - xw), np.minimum(yw, b - yw))
    diag = np.abs(xw * b - yw * a) / np.hypot(a, b)
    dist = np.where(np.isin(win, diagonal_of), np.minimum(dist, diag), dist)
    return np.where(np.isfinite(t[rows, win]), dist, np.inf), win


def _lum(im):
    return im.cpu().numpy().mean(0).reshape(-1)


def _sigma(a, b):
    se = np.sqrt(a.var() / a.size + b.var() / b.size)
    return float(abs(a.mean() - b.mean()) / se)


def _prim_bsdf(desc, prim):
    nq = desc["quads"].size // 9
    table = np.concatenate([desc["bsdf"], desc.get("tri_bsdf", np.zeros(0, np.int32)), [-1]])
    return table[np.where(prim < 0, len(table) - 1, prim)], nq


@pytest.mark.parametrize("K", [16, 512])
def test_cornell_cubes_as_triangles(pkg, oracle, scenes, gpu, plog, K):
    qd = scenes.cornell_box(160, 90)
    md = scenes.cornell_box(160, 90, mesh=("ShortBox", "TallBox"))
    assert md["triangles"].size // 3 == 24 and md["quads"].size // 9 == qd["quads"].size // 9 - 12
    quad_sc, mesh_sc = pkg.Scene(qd), pkg.Scene(md)
    if K == 16:
        # the same surface under every camera ray, but for rays at an edge
        o, d = _camera_rays(qd)
        op, dp = _planes(o, gpu), _planes(d, gpu)
        bq, _ = _prim_bsdf(qd, quad_sc.intersect(op, dp, 1e-2, float("inf"), 0)[0].cpu().numpy())
        for mode in (0, 1):
            bm, nq = _prim_bsdf(md, mesh_sc.intersect(op, dp, 1e-2, float("inf"), mode)[0].cpu().numpy())
            o64, d64 = _camera_rays(qd, float64=True)
            cube_faces = np.arange(5, 17)                     # the quad scene's cube faces (after 5 rectangles)
            dist, _ = _edge_distance64(qd, o64, d64, cube_faces)
            excepted = dist < 1e-4
            print(f"camera rays within 1e-4 of an edge or diagonal: {int(excepted.sum())} of {len(o)}")
            assert excepted.mean() <= 0.01
            assert np.array_equal(bm[~excepted], bq[~excepted])
            assert (bm == list(scenes._BSDFS).index("TallBox")).any()
    tree = _tree(pkg, mesh_sc)
    spp = 64
    uq = _lum(quad_sc.render(tree, None, spp=spp, guided=False, seed=911)[0])
    um_img, verts, _ = mesh_sc.render(tree, None, spp=spp, guided=False, seed=912)
    um = _lum(um_img)
    if K == 16:
        s = plog("mesh_cornell_unguided_vs_quads_sigma", _sigma(um, uq), 4.0, mesh=float(um.mean()), quads=float(uq.mean()))
        assert s < 4.0
        _check_producer(pkg, oracle, tree, verts, 8, 0xC0B, plog, "mesh_unguided")
    node_mix = _train(pkg, mesh_sc, tree, 6, 8, K=K)
    B = len(md["reflectance"]) // 3
    w, m, cov, dif = scenes.diffuse_learned_bsdf(B)
    table = pkg.BsdfTable(w, m, cov, device=gpu, diffuse=dif)
    for what, kw, seed in (("guided", {}, 913), ("product", {"learned_bsdf": table}, 914)):
        img, verts, st = mesh_sc.render(tree, node_mix, spp=spp, guided=True, seed=seed, **kw)
        g = _lum(img)
        assert np.isfinite(g).all() and st["guided_queries"] > 0
        s = plog(f"mesh_cornell_{what}_K{K}_vs_unguided_sigma", _sigma(g, um), 4.0, guided=float(g.mean()),
                 unguided=float(um.mean()))
        assert s < 4.0, (what, g.mean(), um.mean())
    _check_producer(pkg, oracle, tree, verts, 8, 0xC0C, plog, f"mesh_product_K{K}")


# ---- torus scene ---------------------------------------------------------------
def _vertex_prims(pkg, sc, desc, verts, gpu):
    """The primitive under every saved vertex: a ray from the vertex before it
    (the camera for the first) to its position, intersected on the device."""
    rec, nv = verts.to_numpy()
    V = verts.s.max_vertices
    r = rec.reshape(16, V, -1)
    smin, snorm, _, _ = sc.normalization()
    pos = np.stack([r[7 + a] for a in range(3)], -1).astype(np.float64) * snorm + smin       # [V, P, 3]
    prev = np.concatenate([np.broadcast_to(desc["camera_to_world"].reshape(4, 4)[:3, 3], pos[:1].shape), pos[:-1]])
    sel = np.arange(V)[:, None] < nv[None, :]
    o = prev[sel].astype(np.float32)
    d = (pos[sel] - prev[sel]).astype(np.float32)
    prim, t = sc.intersect(_planes(o, gpu), _planes(d, gpu), 1e-3, 1.001, 0)
    return prim.cpu().numpy()


_CHILD = """
import sys
import numpy as np
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
from conftest import load_pkg
import importlib
pkg = load_pkg()
scenes = importlib.import_module("sdmm_mitsuba_amd.scenes")
from test_gpu_li import _tree
sc = pkg.Scene(scenes.torus_scene(160, 90, 24, 12))
img = sc.render(_tree(pkg, sc), None, spp=8, guided=False, seed=4242)[0]
np.save({out!r}, img.cpu().numpy())
"""


@pytest.mark.parametrize("K", [16, 128])
def test_torus_scene(pkg, scenes, gpu, plog, K, tmp_path):
    import torch
    desc = scenes.torus_scene(160, 90, 24, 12)
    sc = pkg.Scene(desc)
    assert sc.n_triangles == 576
    tree = _tree(pkg, sc)
    node_mix = _train(pkg, sc, tree, 6, 8, K=K)
    assert any(m is not None for m in node_mix)
    B = len(desc["reflectance"]) // 3
    w, m, cov, dif = scenes.diffuse_learned_bsdf(B)
    table = pkg.BsdfTable(w, m, cov, device=gpu, diffuse=dif)
    spp = 64
    u_img, verts, _ = sc.render(tree, None, spp=spp, guided=False, seed=5151)
    u = _lum(u_img)
    assert np.isfinite(u).all() and u.mean() > 0
    for what, kw, seed in (("guided", {}, 5152), ("product", {"learned_bsdf": table}, 5153)):
        img, verts, st = sc.render(tree, node_mix, spp=spp, guided=True, seed=seed, **kw)
        g = _lum(img)
        assert np.isfinite(g).all() and st["guided_queries"] > 0
        s = plog(f"mesh_torus_{what}_K{K}_vs_unguided_sigma", _sigma(g, u), 4.0, guided=float(g.mean()),
                 unguided=float(u.mean()))
        assert s < 4.0, (what, g.mean(), u.mean())
    if K != 16:
        return
    # the paths reach the mesh: saved vertices on triangles
    img, verts, _ = sc.render(tree, node_mix, spp=4, guided=True, seed=5154)
    first = img.clone()
    prims = _vertex_prims(pkg, sc, desc, verts, gpu)
    share = float(np.mean(prims >= sc.n_quads))
    print(f"saved vertices on the torus: {100 * share:.1f} % of {prims.size} ({100 * np.mean(prims < 0):.2f} % not found)")
    assert share >= 0.01
    # the same seed renders the same image
    again = sc.render(tree, node_mix, spp=4, guided=True, seed=5154)[0]
    assert torch.equal(first, again)
    # the brute-force loop (SDMM_MESH_BRUTE=1, read at scene creation) in a fresh process
    bvh = sc.render(tree, None, spp=8, guided=False, seed=4242)[0].cpu().numpy()
    out = tmp_path / "brute.npy"
    script = tmp_path / "brute_child.py"
    script.write_text(_CHILD.format(root=str(ROOT), tests=str(ROOT / "tests"), out=str(out)))
    r = subprocess.run([sys.executable, str(script)], env={**os.environ, "SDMM_MESH_BRUTE": "1"}, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.array_equal(np.load(out).view(np.uint32), bvh.view(np.uint32))


# ---- the traversal stack at full depth, edge rays ------------------------------
def _device_equals_host(pkg, gpu, desc, o, d, mint=mf.MINT, maxts=None, sc=None):
    """Scene.intersect mode 0 == mode 1 == intersect_host bitwise on (prim, t
    as bits), at maxt = inf and at a finite maxt (default: the median hit
    distance, which cuts about half the hits).  The host's two modes agree
    first: a device difference is then the device's.  Returns the host's hits
    at maxt = inf."""
    sc = sc or pkg.Scene(mf.camera_fields(desc))
    op, dp = _planes(o, gpu), _planes(d, gpu)
    first = None
    for maxt in (np.inf, None) if maxts is None else maxts:
        if maxt is None:
            maxt = float(np.median(first[1][np.isfinite(first[1])]))
        hp, ht = pkg.intersect_host(desc, o, d, mint, maxt, 0)
        lp, lt = pkg.intersect_host(desc, o, d, mint, maxt, 1)
        assert np.array_equal(hp, lp) and np.array_equal(ht.view(np.uint32), lt.view(np.uint32)), maxt
        for mode in (0, 1):
            prim, t = _bits(*sc.intersect(op, dp, mint, float(maxt), mode))
            bad = np.flatnonzero((prim != hp) | (t != ht.view(np.uint32)))
            assert bad.size == 0, (mode, maxt, bad[:8], prim[bad[:8]], hp[bad[:8]])
        first = first or (hp, ht)
    return first


@pytest.mark.parametrize("which,kind", [("wide", "local"), ("narrow", "local"), ("narrow", "outside"),
                                        ("ladder", "axial")])
def test_deep_mesh_intersect_equals_host_bitwise(pkg, gpu, which, kind):
    """A BVH of 24 inner levels: triangles over six or four decades of size,
    4099 rays (their stacks reach slot 13 or so), and the ladder, whose rays
    fill the LDS stack as far as a tree of 24 levels can (slot 22), in threads
    t and t + 128 of a workgroup at once."""
    if which == "ladder":
        desc, (o, d), mint = mf.ladder_desc(pkg), mf.ladder_rays(), mf.LADDER_MINT
    else:
        desc, (o, d), mint = mf.deep_desc(pkg, which), mf.deep_rays(which, kind), mf.MINT
    hp, ht = _device_equals_host(pkg, gpu, desc, o, d, mint)
    assert (hp >= 0).mean() > 0.9


def test_deep_mesh_batch_sizes(pkg, gpu):
    """Batches smaller than a wave, of one workgroup less and more a ray, and
    with a ragged last block: each ray's answer is its answer in the full batch."""
    desc = mf.deep_desc(pkg, "wide")
    o, d = mf.deep_rays("wide", "local")
    sc = pkg.Scene(mf.camera_fields(desc))
    hp, ht = pkg.intersect_host(desc, o, d, mf.MINT, np.inf, 0)
    for n in (1, 63, 255, 256, 257, 4099):
        # (from the end: the batch of 1 is not the full batch's lane 0)
        oo, dd = o[len(o) - n:], d[len(o) - n:]
        for mode in (0, 1):
            prim, t = _bits(*sc.intersect(_planes(oo, gpu), _planes(dd, gpu), mf.MINT, float("inf"), mode))
            assert prim.shape == (n,)
            assert np.array_equal(prim, hp[len(o) - n:]) and np.array_equal(t, ht[len(o) - n:].view(np.uint32)), (n, mode)


@pytest.mark.parametrize("mint", [1e-4, 1e-3])
def test_hard_rays_intersect_equals_host_bitwise(pkg, scenes, gpu, mint):
    """Grazing rays, rays leaving the surface, -0.0 components, the zero
    direction and non-finite rays among ordinary ones in the same wave."""
    o, d, kinds = mf.hard_rays(scenes)
    hp, ht = _device_equals_host(pkg, gpu, mf.torus_desc(scenes), o, d, mint)
    assert np.all(hp[kinds["special"]] == -1) and np.all(np.isposinf(ht[kinds["special"]]))


def test_flat_grid_and_tie_intersect_equals_host_bitwise(pkg, gpu):
    """Rays through shared vertices and edges (the lowest id), rays in the
    plane (nothing), and a quad against a coplanar triangle at exactly the
    same t (the quad); maxt == t excludes the hit."""
    v, tr = mf.flat_grid()
    desc = mf.base_desc(v, tr, quads=False)
    o, d, expected = mf.flat_grid_rays()
    oi, di = mf.flat_grid_inplane_rays()
    hp, ht = _device_equals_host(pkg, gpu, desc, np.concatenate([o, oi]), np.concatenate([d, di]),
                                 maxts=(np.inf, 1.0, float(np.nextafter(np.float32(1), np.float32(2)))))
    assert np.array_equal(hp[:len(o)], expected) and np.all(ht[:len(o)] == np.float32(1))
    assert np.all(hp[len(o):] == -1)
    o, d, expected = mf.tie_rays()
    hp, ht = _device_equals_host(pkg, gpu, mf.tie_desc(), o, d,
                                 maxts=(np.inf, 1.0, float(np.nextafter(np.float32(1), np.float32(2)))))
    assert np.array_equal(hp, expected)


FURNACE_SPIRAL = (8192, 1e-2, 1e2, 2)      # (the seed: 24 inner levels with the box's 12 triangles; asserted)


def _deep_furnace(scenes):
    """The closed box of emitter triangles of _triangle_furnace round
    spiral_mesh(8192, 1e-2, 1e2) scaled by 0.02 (diffuse, rho 0.6): the Li
    kernels walk a BVH of 24 inner levels."""
    d = _triangle_furnace(scenes, body=False)
    bv, bt, _ = mf.spiral_mesh(*FURNACE_SPIRAL)
    bv = bv * np.float32(0.02)
    v = d["mesh_vertices"].reshape(-1, 3)
    nb = len(d["tri_bsdf"])
    d.update(mesh_vertices=np.concatenate([v, bv]).reshape(-1),
             triangles=np.concatenate([d["triangles"].reshape(-1, 3), bt + len(v)]).reshape(-1),
             tri_bsdf=np.concatenate([d["tri_bsdf"], np.ones(len(bt), np.int32)]),
             tri_emitter=np.concatenate([d["tri_emitter"], np.full(len(bt), -1, np.int32)]),
             tri_flip_normals=np.concatenate([d["tri_flip_normals"], np.zeros(len(bt), np.int32)]))
    assert nb == 12
    return d


_DEEP_CHILD = """
import sys
import numpy as np
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
from conftest import load_pkg
import importlib
pkg = load_pkg()
scenes = importlib.import_module("sdmm_mitsuba_amd.scenes")
from test_gpu_li import _tree
import test_gpu_mesh as tg
sc = pkg.Scene(tg._deep_furnace(scenes))
img = sc.render(_tree(pkg, sc), None, spp=8, guided=False, seed=4343)[0]
np.save({out!r}, img.cpu().numpy())
"""


def test_li_kernels_walk_a_deep_bvh(pkg, scenes, gpu, tmp_path, monkeypatch):
    """The camera and shade kernels' own LDS stack at 24 inner levels: the
    image through the BVH is bitwise the image of the brute-force loop
    (SDMM_MESH_BRUTE=1, read at scene creation) -- unguided against a fresh
    child process, and one guided pass (the MESH shade kernels with guiding)
    against a loop scene created in this process with the same tree and
    mixtures."""
    import torch
    monkeypatch.delenv("SDMM_MESH_BRUTE", raising=False)
    desc = _deep_furnace(scenes)
    assert pkg.mesh_bvh_dump(desc)["levels"] == 24
    # the host's walk and loop agree on the camera rays: a difference below is not the scale envelope's
    o, d = _camera_rays(desc)
    hp, ht = pkg.intersect_host(desc, o, d, 1e-2, np.inf, 0)
    lp, lt = pkg.intersect_host(desc, o, d, 1e-2, np.inf, 1)
    assert np.array_equal(hp, lp) and np.array_equal(ht.view(np.uint32), lt.view(np.uint32))
    assert hp.min() >= 0 and len(np.unique(hp[hp >= 12])) > 50                   # the closed box; many of the body's triangles
    sc = pkg.Scene(desc)
    prim, t = _bits(*sc.intersect(_planes(o, gpu), _planes(d, gpu), 1e-2, float("inf"), 0))
    assert np.array_equal(prim, hp) and np.array_equal(t, ht.view(np.uint32))
    tree = _tree(pkg, sc)
    walk = sc.render(tree, None, spp=8, guided=False, seed=4343)[0].cpu().numpy()
    assert np.isfinite(walk).all() and 0.0 < walk.mean() < 1.0
    out = tmp_path / "brute.npy"
    script = tmp_path / "brute_child.py"
    script.write_text(_DEEP_CHILD.format(root=str(ROOT), tests=str(ROOT / "tests"), out=str(out)))
    r = subprocess.run([sys.executable, str(script)], env={**os.environ, "SDMM_MESH_BRUTE": "1"}, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    loop = np.load(out)
    differ = np.flatnonzero((loop.view(np.uint32) != walk.view(np.uint32)).any(0).reshape(-1))
    assert differ.size == 0, f"{differ.size} pixels differ between the walk and the loop, first {differ[:8]}"
    # guided: the same tree and mixtures on a walk scene and a loop scene
    node_mix = _train(pkg, sc, tree, 4, 8, K=16)
    assert any(m is not None for m in node_mix)
    gw, _, st = sc.render(tree, node_mix, spp=8, guided=True, seed=4344)
    gw = gw.clone()
    assert st["guided_queries"] > 0
    monkeypatch.setenv("SDMM_MESH_BRUTE", "1")
    brute_sc = pkg.Scene(desc)
    monkeypatch.delenv("SDMM_MESH_BRUTE")
    gl, _, sl = brute_sc.render(tree, node_mix, spp=8, guided=True, seed=4344)
    assert torch.equal(gw, gl) and st == sl
    # (the loop scene is the loop: its unguided image is the child's)
    again = brute_sc.render(tree, None, spp=8, guided=False, seed=4343)[0].cpu().numpy()
    assert np.array_equal(again.view(np.uint32), loop.view(np.uint32))
