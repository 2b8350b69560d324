"""GPU: bitmap textures on reflectances in the device Li (sdmm_scene_desc.mesh_uvs,
textures, bsdf_texture; csrc/texture.h).  The CPU oracle's Li knows no
textures, so the yardsticks are the host entry (itself pinned to a numpy
restatement in tests/test_texture_cases.py), exact constructions and analytic
values:

  5. Scene.texture equals texture_host bitwise, at every batch size and mode;
  6. exact inertness: nearest textures whose texels all equal the BSDF's row
     render, record and train bitwise as without textures -- the TEX kernel
     variants against the others, path by path (nearest only: a bilinear sum of
     four equal texels need not round back to the texel);
  7. a flat diffuse surface in the open under a constant sky L: every path
     returns rho(uv) L without variance -- a checker (each pixel one of the two
     products, the one of its texel where its footprint lies inside one), a
     ramp (between the host entry's values at the footprint's corners), a black
     texel (the path ends: no vertex, 0);
  8. guided and product renders of cornell_box(textured=True) agree with the
     BSDF-only one on the mean, the producer equals the oracle;
  9. the BVH image is the brute loop's, with textures;
 10. the mirror twin: a textured probe met from behind gives bitwise the
     mirrored image and records;
 11. a regrown render equals a fresh scene's (the reflectance planes in the
     per-render arena).
"""
import numpy as np
import pytest

import texture_cases as tc
import twosided_fixture as tf
from test_gpu_li import _check_producer, _train, _tree
from test_gpu_scene_regrow import _guide

pytestmark = pytest.mark.gpu
F = np.float32


def _lum(im):
    return im.cpu().numpy().mean(0).reshape(-1)


def _sigma(a, b):
    se = np.sqrt(a.var() / a.size + b.var() / b.size)
    return float(abs(a.mean() - b.mean()) / se)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _saved(verts):
    rec, nv = verts.to_numpy()
    V = verts.s.max_vertices
    return rec.reshape(16, V, -1).copy(), nv.copy(), V


# ---- 5: the device entry against the host entry ------------------------------------------------
@pytest.mark.parametrize("name", tc.GEOMETRIES + ("probe",))
def test_scene_texture_equals_host(pkg, gpu, name):
    import torch
    desc, o, d = tc.probe() if name == "probe" else tc.sweep(name)
    order = np.random.default_rng(3).permutation(len(o))
    o, d = np.ascontiguousarray(o[order]), np.ascontiguousarray(d[order])
    scene = pkg.Scene(tc.camera_fields(desc))
    for mode in (0, 1):
        want = pkg.texture_host(desc, o, d, mode=mode)
        for n in (1, 63, 64, 65, 257, 4099, len(o)):
            if mode == 1 and n == len(o):
                continue
            ot = [torch.from_numpy(o[:n, a].copy()).to(gpu) for a in range(3)]
            dt = [torch.from_numpy(d[:n, a].copy()).to(gpu) for a in range(3)]
            prim, t, uv, rgb = scene.texture(ot, dt, mode=mode)
            torch.cuda.synchronize()
            assert np.array_equal(prim.cpu().numpy(), want[0][:n]), (name, mode, n)
            assert np.array_equal(_bits(t.cpu().numpy()), _bits(want[1][:n])), (name, mode, n)
            got_uv = np.stack([x.cpu().numpy() for x in uv], 1)
            got_rgb = np.stack([x.cpu().numpy() for x in rgb], 1)
            assert np.array_equal(_bits(got_uv), _bits(want[2][:n])), (name, mode, n)
            assert np.array_equal(_bits(got_rgb), _bits(want[3][:n])), (name, mode, n)
    p0, t0 = scene.intersect(ot, dt)
    assert torch.equal(p0, prim) and np.array_equal(_bits(t0.cpu().numpy()), _bits(t.cpu().numpy()))


@pytest.mark.parametrize("mesh", [(), ("ShortBox", "TallBox")], ids=["quads", "mesh"])
def test_scene_texture_of_an_untextured_scene(pkg, scenes, gpu, mesh):
    """A scene with no texture field at all still reports every hit's uv and
    its BSDF's row, bitwise the host entry's -- also on a mesh, which then has
    no per-triangle table on the device."""
    import torch
    desc = scenes.cornell_box(16, 9, mesh=mesh)
    assert "textures" not in desc and "mesh_uvs" not in desc
    o, d = tf.camera_rays({**desc, "width": 64, "height": 36})
    want = pkg.texture_host(desc, o, d)
    n_quads = desc["quads"].size // 9
    assert ((want[0] >= n_quads).sum() > 100) == bool(mesh) and (want[0] >= 0).sum() > 1000 and (want[0] < 0).any()
    scene = pkg.Scene(desc)
    for mode in (0, 1):
        prim, t, uv, rgb = scene.texture([torch.from_numpy(o[:, a].copy()).to(gpu) for a in range(3)],
                                         [torch.from_numpy(d[:, a].copy()).to(gpu) for a in range(3)], mode=mode)
        assert np.array_equal(prim.cpu().numpy(), want[0]) and np.array_equal(_bits(t.cpu().numpy()), _bits(want[1]))
        assert np.array_equal(_bits(np.stack([x.cpu().numpy() for x in uv], 1)), _bits(want[2])), mode
        assert np.array_equal(_bits(np.stack([x.cpu().numpy() for x in rgb], 1)), _bits(want[3])), mode


# ---- 6: exact inertness ------------------------------------------------------------------------
def _constant_textures(desc, rnd):
    """desc with every BSDF of kind 0, 1 or 3 under a nearest texture whose
    texels all equal its reflectance row: 1 x 1 and 3 x 5 by turns, wrap modes
    by BSDF and `rnd` (over rnd = 0 .. 4 every BSDF meets every mode on both
    axes); the lookups leave [0, 1) where the wrap brings the texel back
    (repeat, clamp, mirror) and stay inside under zero and one."""
    refl = np.asarray(desc["reflectance"], F).reshape(-1, 3)
    bp = desc.get("bsdf_params")
    kinds = np.zeros(len(refl)) if bp is None else np.asarray(bp).reshape(-1, 8)[:, 0]
    texs, bt = [], np.full(len(refl), -1, np.int32)
    for b in range(len(refl)):
        if kinds[b] not in (0, 1, 3):
            continue
        w, h = ((1, 1), (3, 5))[(b + rnd) % 2]
        wu, wv = (b + rnd) % 5, (2 * b + rnd) % 5
        inside = wu >= 3 or wv >= 3
        texs.append({"pixels": np.broadcast_to(refl[b], (h, w, 3)).copy(), "filter": 1, "wrap_u": wu, "wrap_v": wv,
                     "uv_scale": (0.5, 0.5) if inside else (3.0, -2.0), "uv_offset": (0.25, 0.25) if inside else (-1.0, 0.5)})
        bt[b] = len(texs) - 1
    return {**desc, "textures": texs, "bsdf_texture": bt}


def _render_all(pkg, scene, tree, mixes, table, seed):
    """The unguided, guided and product renders: image, counts, saved vertices, producer output."""
    import torch
    out = []
    for what, kw in (("unguided", {}), ("guided", dict(node_mix=mixes, guided=True)),
                     ("product", dict(node_mix=mixes, guided=True, learned_bsdf=table))):
        img, verts, st = scene.render(tree, spp=2, seed=seed, **kw)
        img = img.clone()
        r, nv, V = _saved(verts)
        prod = tree.push_training(verts, 8, seed + 1)
        torch.cuda.synchronize()
        out.append((what, img, st, r, nv, V, prod))
    return out


def _assert_same_renders(a, b):
    import torch
    for (what, ia, sa, ra, na, V, pa), (_, ib, sb, rb, nb, _, pb) in zip(a, b):
        assert torch.equal(ia, ib) and np.array_equal(_bits(ia.cpu().numpy()), _bits(ib.cpu().numpy())), what
        assert sa == sb and np.array_equal(na, nb), what
        sel = np.arange(V)[:, None] < na[None, :]
        for f in range(16):
            assert np.array_equal(_bits(ra[f][sel]), _bits(rb[f][sel])), (what, f)
        for k, v in pa.items():
            if isinstance(v, list):
                assert all(torch.equal(x, y) for x, y in zip(v, pb[k])), (what, k)
            elif isinstance(v, torch.Tensor):
                assert torch.equal(v, pb[k]), (what, k)
            else:
                assert np.array_equal(v, pb[k]), (what, k)
        assert pa["w"].numel() > 0 and (what == "unguided" or sa["guided_queries"] > 0)


INERT = {
    "quads": lambda s: s.cornell_box(32, 18, plastic=("TallBox", "Floor"), phong=("ShortBox", "BackWall")),
    "mesh_diffuse": lambda s: s.sheet_scene(32, 18, nx=4, nz=8, material="diffuse"),
    "mesh_plastic": lambda s: s.sheet_scene(32, 18, nx=4, nz=8, material="plastic"),
    "mesh_phong": lambda s: s.sheet_scene(32, 18, nx=4, nz=8, material="phong"),
    "mesh_diffuse_normals": lambda s: s.sheet_scene(32, 18, nx=4, nz=8, material="diffuse", smooth_normals=True),
    "mesh_plastic_normals": lambda s: s.sheet_scene(32, 18, nx=4, nz=8, material="plastic", smooth_normals=True),
    "mesh_phong_normals": lambda s: s.sheet_scene(32, 18, nx=4, nz=8, material="phong", smooth_normals=True),
}


@pytest.mark.parametrize("name", list(INERT))
def test_constant_textures_are_inert(pkg, scenes, synth, gpu, name):
    desc = INERT[name](scenes)
    if "triangles" in desc:
        # the sheet's own uvs in one round, the test's (u, v) in the others
        uvs = scenes.sheet_mesh(4, 8, uvs=True)[-1].reshape(-1)
    plain = pkg.Scene(desc)
    tree, mixes = _guide(pkg, synth, plain)
    learned = scenes.diffuse_learned_bsdf(len(desc["reflectance"]) // 3)
    table = pkg.BsdfTable(*learned[:3], device=gpu, diffuse=learned[3])
    want = _render_all(pkg, plain, tree, mixes, table, 90)
    assert float(want[0][1].mean()) > 0
    for rnd in range(5):
        tdesc = _constant_textures(desc, rnd)
        if "triangles" in desc and rnd == 1:
            tdesc["mesh_uvs"] = uvs
        assert (tdesc["bsdf_texture"] >= 0).sum() >= 3
        _assert_same_renders(_render_all(pkg, pkg.Scene(tdesc), tree, mixes, table, 90), want)


# ---- 7: rho(uv) L on a flat surface in the open ---------------------------------------------------
SKY = (1.5, 2.25, 0.75)
RHO_A, RHO_B = (0.625, 0.5, 0.375), (0.25, 0.75, 0.125)
W7, H7 = 32, 18


def _flat(scenes, geometry, tex, origin=(0.5, 1.2, 0.5)):
    """One unit square (tc.sweep) under the texture and a constant sky, seen
    from above by a camera whose every pixel lies on it; two-sided: the
    square's winding faces down."""
    desc, _, _ = tc.sweep(geometry, [tex])
    desc = tc.camera_fields(desc, W7, H7, origin=origin)
    return {**desc, "bsdf_twosided": np.ones(1, np.int32), **scenes.constant_environment(SKY)}


def _corner_lookups(pkg, desc):
    """texture_host through every pixel's four corners: (uv [H, W, 4, 2], rgb [H, W, 4, 3])."""
    W, H = desc["width"], desc["height"]
    cam = np.asarray(desc["camera_to_world"], np.float64).reshape(4, 4)[:3]
    tanx = np.tan(0.5 * np.radians(desc["fov_x_deg"]))
    SX, SY = np.meshgrid(np.arange(W + 1) / W, np.arange(H + 1) / H)
    l = np.stack([(1 - 2 * SX) * tanx, (1 - 2 * SY) * tanx / (W / H), np.ones_like(SX)], -1).reshape(-1, 3)
    d = l @ cam[:, :3].T
    o = np.broadcast_to(cam[:, 3], d.shape)
    prim, _, uv, rgb = pkg.texture_host(desc, o, d)
    assert (prim >= 0).all()
    uv, rgb = uv.reshape(H + 1, W + 1, 2), rgb.reshape(H + 1, W + 1, 3)
    pick = lambda a: np.stack([a[:-1, :-1], a[:-1, 1:], a[1:, :-1], a[1:, 1:]], 2)
    return pick(uv), pick(rgb)


@pytest.mark.parametrize("geometry", ["quad", "mesh_uv", "mesh_bary"])
def test_checker_on_a_flat_surface(pkg, scenes, gpu, geometry):
    tex = scenes.checker_texture(4, 4, RHO_A, RHO_B)
    desc = _flat(scenes, geometry, tex)
    scene = pkg.Scene(desc)
    img, verts, st = scene.render(_tree(pkg, scene), None, spp=1, max_depth=3, guided=False, seed=31)
    img = img.cpu().numpy().astype(np.float64)                          # [3, H, W]
    _, nv, _ = _saved(verts)
    assert (nv == 1).all()
    prod = [np.asarray(F(r) * F(SKY), np.float64) for r in (RHO_A, RHO_B)]
    rel = [np.abs(img - p[:, None, None]).max(0) / p.min() for p in prod]
    print(f"checker on {geometry}: largest relative distance to the nearer product {np.minimum(*rel).max():.3g}; "
          f"{int((rel[0] <= 1e-6).sum())} pixels of colour a, {int((rel[1] <= 1e-6).sum())} of b")
    assert (np.minimum(*rel) <= 1e-6).all()
    assert (rel[0] <= 1e-6).sum() > 100 and (rel[1] <= 1e-6).sum() > 100
    # a footprint inside one texel: that texel's product
    uv, rgb = _corner_lookups(pkg, desc)
    sc, of = np.asarray(tex.get("uv_scale", 1.0), F), np.asarray(tex.get("uv_offset", 0.0), F)
    cell = np.floor((uv * sc + of) * F(4.0))
    inside = (cell == cell[:, :, :1]).all((2, 3))
    assert inside.mean() > 0.5 and (~inside).sum() > 20
    want = rgb[:, :, 0].astype(np.float64) * np.asarray(SKY, F).astype(np.float64)      # [H, W, 3]
    err = np.abs(img.transpose(1, 2, 0) - want).max(2) / want.min()
    print(f"checker on {geometry}: {int(inside.sum())} pixels inside one texel, largest relative error {err[inside].max():.3g}")
    assert (err[inside] <= 1e-6).all()


# the whole square from 1.2 above its centre; from 0.5 above, the images lie inside the triangle x > z and inside z > x
RAMP_VIEWS = {"whole": (0.5, 1.2, 0.5), "first": (0.7, 0.5, 0.3), "second": (0.3, 0.5, 0.7)}


@pytest.mark.parametrize("geometry,view", [(g, v) for g in ("quad", "mesh_uv", "mesh_bary") for v in RAMP_VIEWS
                                           if (g, v) != ("mesh_bary", "whole")])
def test_ramp_on_a_flat_surface(pkg, scenes, gpu, geometry, view):
    """Each pixel between the host entry's values at its footprint's corners:
    a ramp's channel is monotone along one texture coordinate, and its.uv is
    linear over a primitive, so over a footprint on one primitive the extremes
    are at the corners.  Without mesh_uvs a triangle's uv is its own (u, v),
    which jumps across the square's diagonal: a footprint that straddles it is
    not bounded by its corners (the whole view measured 0.0587 relative above
    them there), so that mesh is seen through the two views that each lie on
    one triangle; the others through all three."""
    tex = scenes.ramp_texture(3, 5)
    assert tex["filter"] == "bilinear" and tex["wrap_u"] == tex["wrap_v"] == "clamp"
    desc = _flat(scenes, geometry, tex, RAMP_VIEWS[view])
    if geometry != "quad" and view != "whole":
        o, d = tf.camera_rays(desc)
        assert set(pkg.texture_host(desc, o, d)[0]) == {0 if view == "first" else 1}
    scene = pkg.Scene(desc)
    img, verts, st = scene.render(_tree(pkg, scene), None, spp=1, max_depth=3, guided=False, seed=32)
    img = img.cpu().numpy().astype(np.float64).transpose(1, 2, 0)       # [H, W, 3]
    _, rgb = _corner_lookups(pkg, desc)
    L = np.asarray(SKY, F).astype(np.float64)
    lo, hi = rgb.min(2).astype(np.float64) * L, rgb.max(2).astype(np.float64) * L
    below, above = (lo - img) / lo, (img - hi) / hi
    print(f"ramp on {geometry}: largest relative excursion below {below.max():.3g}, above {above.max():.3g}; "
          f"{len(np.unique(_bits(img.astype(F))[:, :, 0]))} distinct reds")
    assert (below <= 1e-6).all() and (above <= 1e-6).all()
    assert len(np.unique(_bits(img.astype(F))[:, :, 0])) > 100             # a ramp, not two colours (mesh_uv: clamped outside [0, 1])


@pytest.mark.parametrize("geometry", ["quad", "mesh_uv", "mesh_bary"])
def test_black_texel_ends_the_path(pkg, scenes, gpu, geometry):
    tex = scenes.checker_texture(4, 4, RHO_A, (0.0, 0.0, 0.0))
    desc = _flat(scenes, geometry, tex)
    scene = pkg.Scene(desc)
    img, verts, st = scene.render(_tree(pkg, scene), None, spp=1, max_depth=3, guided=False, seed=33)
    img = img.cpu().numpy().reshape(3, -1)
    _, nv, _ = _saved(verts)
    black = img.max(0) == 0
    assert black.sum() > 100 and (~black).sum() > 100
    assert np.array_equal(black, nv == 0) and np.array_equal(~black, nv == 1)
    want = np.asarray(F(RHO_A) * F(SKY), np.float64)
    assert (np.abs(img[:, ~black] - want[:, None]).max(0) / want.min() <= 1e-6).all()
    # and the black pixels are those the host entry finds black at the pixel centre
    o, d = tf.camera_rays(desc)
    centre = pkg.texture_host(desc, o, d)[3].max(1) == 0
    uv, rgb = _corner_lookups(pkg, desc)
    same = (rgb == rgb[:, :, :1]).all((2, 3)).reshape(-1)               # footprints of one colour
    assert np.array_equal(black[same], centre[same])


# ---- 8: guided and product renders of the textured box ---------------------------------------------
SW, SH = 48, 27


def test_textured_box_guided_and_product_unbiased(pkg, oracle, scenes, gpu, plog):
    import torch
    desc = scenes.cornell_box(SW, SH, textured=True)
    scene = pkg.Scene(desc)
    tree = _tree(pkg, scene)
    node_mix = _train(pkg, scene, tree, 4, 8, K=16)
    assert any(m is not None for m in node_mix)
    B = len(desc["reflectance"]) // 3
    w, m, cov, dif = scenes.diffuse_learned_bsdf(B)
    table = pkg.BsdfTable(w, m, cov, device=gpu, diffuse=dif)
    for tag, kw in (("textured_box_guided", {}), ("textured_box_product", {"learned_bsdf": table})):
        img, verts, st = scene.render(tree, node_mix, spp=4, guided=True, seed=77, **kw)
        assert np.isfinite(img.cpu().numpy()).all() and st["guided_queries"] > 0
        _check_producer(pkg, oracle, tree, verts, 8, 0xAD0, plog, tag)
    spp = 64
    u_img = scene.render(tree, None, spp=spp, guided=False, seed=4330)[0].clone()
    u = _lum(u_img)
    for what, kw, seed in (("guided", {}, 2360), ("product", {"learned_bsdf": table}, 2361)):
        g = _lum(scene.render(tree, node_mix, spp=spp, guided=True, seed=seed, **kw)[0])
        assert np.isfinite(g).all()
        s = plog(f"li_textured_box_{what}_vs_unguided_mean_sigma", _sigma(g, u), 4.0, guided=float(g.mean()),
                 unguided=float(u.mean()))
        print(f"textured box {what}: mean {g.mean():.5f} against BSDF-only {u.mean():.5f} ({s:.2f} sigma)")
        assert s < 4.0, (what, g.mean(), u.mean())
    bare = {k: v for k, v in desc.items() if k not in ("textures", "bsdf_texture")}
    p_img = pkg.Scene(bare).render(tree, None, spp=spp, guided=False, seed=4330)[0]
    assert not torch.equal(u_img, p_img)


# ---- 9: BVH == brute ---------------------------------------------------------------------------------
@pytest.mark.parametrize("normals", [False, True])
def test_textured_bvh_equals_brute(pkg, scenes, gpu, monkeypatch, normals):
    import torch
    monkeypatch.delenv("SDMM_MESH_BRUTE", raising=False)
    desc = scenes.sheet_scene(48, 27, nx=8, nz=24, texture=scenes.checker_texture(8, 8), smooth_normals=normals)
    scene = pkg.Scene(desc)
    tree = _tree(pkg, scene)
    a, va, st = scene.render(tree, None, spp=4, guided=False, seed=606)
    a = a.clone()
    ra, na, _ = _saved(va)
    monkeypatch.setenv("SDMM_MESH_BRUTE", "1")
    brute = pkg.Scene(desc)
    monkeypatch.delenv("SDMM_MESH_BRUTE")
    b, vb, sb = brute.render(tree, None, spp=4, guided=False, seed=606)
    rb, nb, V = _saved(vb)
    assert torch.equal(a, b) and st == sb and np.isfinite(a.cpu().numpy()).all() and float(a.mean()) > 0
    sel = np.arange(V)[:, None] < na[None, :]
    assert np.array_equal(na, nb) and all(np.array_equal(_bits(ra[f][sel]), _bits(rb[f][sel])) for f in range(16))
    # the texture is seen: the same scene without it renders another image
    bare = {k: v for k, v in desc.items() if k not in ("textures", "bsdf_texture", "mesh_uvs")}
    c = pkg.Scene(bare).render(tree, None, spp=4, guided=False, seed=606)[0]
    assert not torch.equal(a, c)


# ---- 10: the mirror twin ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1, 3])
def test_mirror_twin_with_a_textured_probe(pkg, scenes, gpu, kind):
    A, _ = tf.twin_scenes(scenes, kind)
    A["textures"] = [scenes.ramp_texture(3, 5, wrap_u="mirror", wrap_v="repeat", uv_scale=(1.5, -2.0), uv_offset=(0.25, 0.125)),
                     scenes.checker_texture(4, 4, RHO_A, RHO_B)]
    A["bsdf_texture"] = np.asarray([-1, kind % 2], np.int32)
    B = scenes.mirror_z(A, keep=(tf.PROBE,))
    B["bsdf_twosided"] = np.asarray([0, 1], np.int32)
    out = []
    for desc in (A, B):
        scene = pkg.Scene(desc)
        img, verts, st = scene.render(_tree(pkg, scene), None, spp=1, max_depth=3, guided=False, seed=800 + kind)
        r, nv, V = _saved(verts)
        out.append((img.cpu().numpy().copy(), r, nv, st))
    (ia, ra, na, sa), (ib, rb, nb, sb) = out
    assert sa == sb and np.array_equal(na, nb) and (na >= 1).sum() > 0.6 * na.size
    assert np.array_equal(_bits(ia), _bits(ib)) and (ia.reshape(3, -1).max(0) > 0).mean() > 0.6
    sel = np.arange(ra.shape[1])[:, None] < na[None, :]
    for f in range(16):
        a, b = ra[f][sel], rb[f][sel]
        if f == 9:
            # c.z = (p.z - scene_min.z) / norm, p.z about 0 of either sign: not a mirrored quantity
            assert np.abs(a - b).max(initial=0.0) <= 1e-6
        elif f in (12, 15):
            assert np.array_equal(_bits(a), _bits(-b)), f
        elif f in (13, 14):
            assert np.array_equal(a, b) and (a == 0).all(), f           # zeros of either sign (A saves n, B -n)
        else:
            assert np.array_equal(_bits(a), _bits(b)), f
    # the probe's colour varies over the image: the texture, not the row
    plain = {k: v for k, v in A.items() if k not in ("textures", "bsdf_texture")}
    scene = pkg.Scene(plain)
    ip = scene.render(_tree(pkg, scene), None, spp=1, max_depth=3, guided=False, seed=800 + kind)[0].cpu().numpy()
    assert not np.array_equal(ip, ia)


# ---- 11: regrown buffers ---------------------------------------------------------------------------
RW, RH = 16, 9
SEQUENCE = [(1, 3), (4, 3), (4, 6), (1, 3)]


def _render_bytes(scene, tree, mixes, table, spp, saved, step, gpu):
    import torch
    img = torch.zeros(3, RH, RW, device=gpu)
    sqr = torch.zeros(3, RH, RW, device=gpu)
    kw = dict(node_mix=mixes, guided=True, learned_bsdf=table) if mixes is not None else {}
    _, verts, st = scene.render(tree, spp=spp, max_depth=saved + 1, saved_vertices=saved, seed=40 + step,
                                image=img, image_sqr=sqr, **kw)
    rec, nv = verts.to_numpy()
    P = RW * RH * spp
    assert st["paths"] == P == nv.size
    rec = rec.reshape(16, saved, P)
    used = np.arange(saved)[:, None] < nv[None, :]
    return (img.cpu().numpy().tobytes(), sqr.cpu().numpy().tobytes(), nv.tobytes(), rec[:, used].tobytes(),
            st["segments"], st["guided_queries"])


@pytest.mark.parametrize("guided", [False, True], ids=["unguided", "product"])
@pytest.mark.parametrize("name", ["box", "sheet_normals"])
def test_regrown_textured_render_equals_a_fresh_scene(pkg, scenes, synth, gpu, name, guided):
    if name == "box":
        desc = scenes.cornell_box(RW, RH, textured=True)
    else:
        desc = scenes.sheet_scene(RW, RH, nx=4, nz=8, material="plastic", texture=scenes.ramp_texture(3, 5),
                                  smooth_normals=True)
    scene = pkg.Scene(desc)
    tree, mixes = _guide(pkg, synth, scene)
    table = None
    if guided:
        learned = scenes.diffuse_learned_bsdf(len(desc["reflectance"]) // 3)
        table = pkg.BsdfTable(*learned[:3], device=gpu, diffuse=learned[3])
    else:
        mixes = None
    for step, (spp, saved) in enumerate(SEQUENCE):
        got = _render_bytes(scene, tree, mixes, table, spp, saved, step, gpu)
        want = _render_bytes(pkg.Scene(desc), tree, mixes, table, spp, saved, step, gpu)
        for what, a, b in zip(("image", "image_sqr", "nv", "saved vertices", "segments", "guided queries"), got, want):
            assert a == b, (name, guided, step, what)
        assert any(got[3]) and got[4] > 0
