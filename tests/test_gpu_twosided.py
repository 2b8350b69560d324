"""GPU: the single-child `twosided` adapter in the device Li
(sdmm_scene_desc.bsdf_twosided; bsdfs/twosided.cpp).

  * front hits are inert: the Cornell box with the flag on every BSDF renders
    bitwise what the plain box renders, records and stats included;
  * the mirror twin: a probe met from behind in the mirrored scene gives
    bitwise the mirrored image and records of the probe met from the front --
    the bounce runs in (s, t, -n) of Frame(n), the saved vertex carries -n;
  * a flat sheet under a constant environment is rho * L from both sides, and
    black from behind without the flag;
  * sheet_scene, where back hits dominate: the guided and the product render
    agree with the BSDF-only one on the mean, the producer equals the oracle on
    records carrying flipped normals, a two-sided conductor's learned model is
    conditioned on hits from behind, and the BVH image is the brute loop's.
"""
import numpy as np
import pytest

import twosided_fixture as tf
from test_gpu_li import _check_producer, _train, _tree

pytestmark = pytest.mark.gpu


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
    return rec.reshape(16, V, -1), nv, V


# ---- 4: inert on front hits ----------------------------------------------------------
def test_front_hits_are_inert(pkg, scenes, gpu):
    import torch
    W, H = 64, 36
    names = tuple(scenes._BSDFS)
    plain_desc = scenes.cornell_box(W, H)
    flagged_desc = scenes.cornell_box(W, H, twosided=names)
    assert flagged_desc["bsdf_twosided"].all()
    plain, flagged = pkg.Scene(plain_desc), pkg.Scene(flagged_desc)
    tree = _tree(pkg, plain)
    node_mix = _train(pkg, plain, tree, 2, 8, K=16)
    assert any(m is not None for m in node_mix)
    for guided in (False, True):
        kw = dict(spp=2, guided=guided, seed=31 + guided)
        a, va, sa = plain.render(tree, node_mix if guided else None, **kw)
        a = a.clone()
        ra, na, V = _saved(va)
        ra, na = ra.copy(), na.copy()
        b, vb, sb = flagged.render(tree, node_mix if guided else None, **kw)
        rb, nb, _ = _saved(vb)
        assert torch.equal(a, b) and sa == sb and np.array_equal(na, nb) and na.sum() > W * H
        sel = np.arange(V)[:, None] < na[None, :]
        for f in range(16):
            assert np.array_equal(_bits(ra[f][sel]), _bits(rb[f][sel])), f
        if guided:
            assert sa["guided_queries"] > 0
        # the box is closed: no path meets a back side, so no saved normal is the negated face normal
        smin, snorm, _, _ = flagged.normalization()
        p, _, n = tf.vertex_table(rb.reshape(-1), nb, V, smin, snorm)
        side = tf.quad_sides(flagged_desc, p, n)
        assert (side == 1).mean() > 0.99 and not (side == -1).any()


# ---- 5: the mirror twin ---------------------------------------------------------------
def _twin_check(pkg, scenes, kind, w, h, pixels, seed):
    import torch
    A, B = tf.twin_scenes(scenes, kind, w, h)
    out = []
    for desc in (A, B):
        sc = pkg.Scene(desc)
        img, verts, st = sc.render(_tree(pkg, sc), None, spp=1, max_depth=3, guided=False, seed=seed, pixels=pixels)
        r, nv, V = _saved(verts)
        out.append((img.cpu().numpy().copy(), r.copy(), nv.copy(), st))
    (ia, ra, na, sa), (ib, rb, nb, sb) = out
    n_paths = w * h if pixels is None else pixels[1] - pixels[0]
    assert sa["paths"] == n_paths and sa == sb, (sa, sb)
    assert np.array_equal(na, nb)
    lit = (ia.reshape(3, -1).max(0) > 0).sum()
    assert lit >= 0.9 * n_paths, lit                        # the probe reflects an emitter nearly everywhere
    assert np.array_equal(_bits(ia), _bits(ib))
    V = ra.shape[1]
    sel = np.arange(V)[:, None] < na[None, :]
    for f in range(16):
        a, b = ra[f][sel], rb[f][sel]
        if f == 9:
            # c.z = (p.z - scene_min.z) / norm, p.z about 0 of either sign: not a mirrored quantity
            assert np.abs(a - b).max(initial=0.0) <= 1e-6
        elif f in (12, 15):
            assert np.array_equal(_bits(a), _bits(-b)), f
        elif f in (13, 14):
            assert np.array_equal(a, b) and (a == 0).all(), f           # zeros of either sign
        else:
            assert np.array_equal(_bits(a), _bits(b)), f
    if sel.any():
        assert (ra[15][sel] == 1.0).all() and (rb[15][sel] == -1.0).all()   # A saves n, B saves -n
    return na, sa


@pytest.mark.parametrize("kind", tf.TWIN_KINDS)
def test_mirror_twin(pkg, scenes, gpu, kind):
    nv, st = _twin_check(pkg, scenes, kind, tf.TWIN_W, tf.TWIN_H, None, 900 + kind)
    n = tf.TWIN_W * tf.TWIN_H
    if kind == 1:
        # both lobes of the plastic are reached: the delta lobe saves no vertex
        assert 0.02 * n < (nv == 0).sum() and (nv == 1).sum() > 0.5 * n
    elif kind == 6:
        assert (nv == 0).all() and st["segments"] == n              # delta only: no vertex, the ray still traced
    else:
        assert (nv == 1).sum() > 0.9 * n


def test_mirror_twin_across_blocks(pkg, scenes, gpu):
    """4099 paths of the Phong twin: more than sixteen 256-thread blocks and a tail."""
    nv, _ = _twin_check(pkg, scenes, 3, 128, 64, (5, 5 + 4099), 77)
    assert len(nv) == 4099 and (nv == 1).sum() > 3600


# ---- 6: a flat sheet under a constant environment ---------------------------------------
def test_flat_sheet_in_constant_environment(pkg, scenes, gpu):
    W, H = 48, 27
    imgs, info = {}, {}
    for two in (True, False):
        desc = tf.flat_sheet(scenes, two, W, H)
        sc = pkg.Scene(desc)
        img, verts, st = sc.render(_tree(pkg, sc), None, spp=1, max_depth=3, guided=False, seed=66)
        r, nv, V = _saved(verts)
        imgs[two] = img.cpu().numpy().reshape(3, -1).copy()
        info[two] = (r.copy(), nv.copy(), sc.normalization())
    r, nv, (smin, snorm, _, _) = info[True]
    hit = nv == 1
    x = r[7][0].astype(np.float64) * snorm + smin[0]          # spp 1: path = pixel
    front, back = hit & (x < 0), hit & (x > 0)
    assert front.sum() > 100 and back.sum() > 100 and (nv <= 1).all()
    want = np.float32(tf.SHEET_RHO) * np.float32(tf.SHEET_L)  # one float product per channel
    sheet = imgs[True][:, hit]
    rel = np.abs(sheet.astype(np.float64) - want[:, None]) / want[:, None]
    print(f"flat sheet: {int(front.sum())} front and {int(back.sum())} back pixels, largest relative error {rel.max():.3g}")
    assert rel.max() <= 1e-6
    # back-side pixels are bitwise the front-side pixels' value
    for ch in range(3):
        assert len(np.unique(_bits(imgs[True][ch, hit]))) == 1
    assert np.array_equal(_bits(imgs[True][:, back][:, :1]), _bits(imgs[True][:, front][:, :1]))
    # pixels beside the sheet see the environment itself
    assert np.array_equal(imgs[True][:, ~hit], np.broadcast_to(np.float32(tf.SHEET_L)[:, None], (3, int((~hit).sum()))))
    # both saved normals face the camera: the face normal in front, its negation behind
    assert (r[14][0][hit] == 1.0).all()
    # one-sided: black from behind, the rest untouched
    assert (imgs[False][:, back] == 0).all() and (info[False][1][back] == 0).all()
    assert np.array_equal(_bits(imgs[False][:, ~back]), _bits(imgs[True][:, ~back]))


# ---- 7, 8: guided and product renders where back hits dominate ----------------------------
SW, SH = 48, 27


def _sheet_vertices(desc, sc, verts):
    r, nv, V = _saved(verts)
    smin, snorm, _, _ = sc.normalization()
    p, _, n = tf.vertex_table(r.reshape(-1), nv, V, smin, snorm)
    on = tf.on_sheet(desc, p)
    return on, n


@pytest.mark.parametrize("material", ["phong", "diffuse"])
def test_sheet_guided_and_product_unbiased(pkg, oracle, scenes, gpu, plog, material):
    desc = scenes.sheet_scene(SW, SH, material=material)
    b = int(desc["tri_bsdf"][0])
    assert desc["bsdf_twosided"][b] == 1 and (material != "phong" or desc["learned_models_nd"][b] is not None)
    sc = pkg.Scene(desc)
    tree = _tree(pkg, sc)
    node_mix = _train(pkg, sc, tree, 4, 8, K=16)
    assert any(m is not None for m in node_mix)
    B = len(desc["reflectance"]) // 3
    w, m, cov, dif = scenes.diffuse_learned_bsdf(B)
    table = pkg.BsdfTable(w, m, cov, device=gpu, diffuse=dif)
    for tag, kw in ((f"sheet_{material}_guided", {}), (f"sheet_{material}_product", {"learned_bsdf": table})):
        img, verts, st = sc.render(tree, node_mix, spp=4, guided=True, seed=77, **kw)
        assert np.isfinite(img.cpu().numpy()).all() and st["guided_queries"] > 0
        # the records the producer reads carry flipped normals: at least 30 % of the sheet's
        on, n = _sheet_vertices(desc, sc, verts)
        share = float((n[on, 1] < 0).mean())
        plog(f"{tag}_back_vertex_share", share, 0.30, lower=True, sheet_vertices=int(on.sum()))
        print(f"{tag}: {int(on.sum())} saved vertices on the sheet, {share:.3f} of them with the negated face normal")
        assert on.sum() > 1000 and share >= 0.30
        _check_producer(pkg, oracle, tree, verts, 8, 0xAD0, plog, tag)
    spp = 64
    u = _lum(sc.render(tree, None, spp=spp, guided=False, seed=4330)[0])
    for what, kw, seed in (("guided", {}, 2360), ("product", {"learned_bsdf": table}, 2361)):
        g = _lum(sc.render(tree, node_mix, spp=spp, guided=True, seed=seed, **kw)[0])
        assert np.isfinite(g).all()
        s = plog(f"li_sheet_{material}_{what}_vs_unguided_mean_sigma", _sigma(g, u), 4.0, guided=float(g.mean()),
                 unguided=float(u.mean()))
        print(f"sheet {material} {what}: mean {g.mean():.5f} against BSDF-only {u.mean():.5f} ({s:.2f} sigma)")
        assert s < 4.0, (what, g.mean(), u.mean())


def test_sheet_product_rows_from_behind(pkg, scenes, gpu):
    """A two-sided rough conductor that paths meet from behind only: in the
    open scene the patch lies face up above everything else, and only the sky
    is above it.  A product pass conditions its learned SDMM4 on the flipped
    local wi: the image is finite and differs from the same pass without the
    model (the plain conditional there), which it could not if a back hit got
    no usable row of the product table -- every hit on the patch is one."""
    import torch
    desc = scenes.sheet_scene(SW, SH, patch=True, environment=scenes.constant_environment((1.0, 0.9, 0.8)))
    B = len(desc["reflectance"]) // 3
    patch = B - 1
    assert desc["bsdf_params"][8 * patch] == 2.0 and desc["bsdf_twosided"][patch] == 1
    assert desc["learned_models"][patch] is not None
    sc = pkg.Scene(desc)
    tree = _tree(pkg, sc)
    node_mix = _train(pkg, sc, tree, 3, 8, K=16)
    assert any(m is not None for m in node_mix)
    w, m, cov, dif = scenes.diffuse_learned_bsdf(B)
    table = pkg.BsdfTable(w, m, cov, device=gpu, diffuse=dif)
    kw = dict(spp=16, guided=True, seed=91, learned_bsdf=table)
    a, verts, st = sc.render(tree, node_mix, **kw)
    a = a.clone()
    assert np.isfinite(a.cpu().numpy()).all() and st["guided_queries"] > 0

    def on_patch(sc_, verts_):
        r, nv, V = _saved(verts_)
        smin, snorm, _, _ = sc_.normalization()
        p, _, n = tf.vertex_table(r.reshape(-1), nv, V, smin, snorm)
        on = np.abs(p[:, 1] - 3.2) < 1e-3                   # nothing else meets that plane
        return on, n
    on, n = on_patch(sc, verts)
    print(f"patch: {int(on.sum())} saved vertices, all from behind: {bool((n[on, 1] == -1.0).all())}")
    assert on.sum() > 50 and (n[on, 1] == -1.0).all()       # the negated face normal (0, 1, 0)
    bare = pkg.Scene(dict(desc, learned_models=[None] * B))
    c = bare.render(tree, node_mix, **kw)[0]
    assert np.isfinite(c.cpu().numpy()).all() and not torch.equal(a, c)
    # one-sided, the patch ends every path that reaches it: no vertex there
    one = pkg.Scene({k: v for k, v in desc.items() if k != "bsdf_twosided"})
    on1, _ = on_patch(one, one.render(tree, node_mix, **kw)[1])
    assert not on1.any()


# ---- 9: BVH == brute ------------------------------------------------------------------------
def test_sheet_bvh_equals_brute(pkg, scenes, gpu, monkeypatch):
    import torch
    monkeypatch.delenv("SDMM_MESH_BRUTE", raising=False)
    desc = scenes.sheet_scene(64, 36)
    sc = pkg.Scene(desc)
    tree = _tree(pkg, sc)
    a, _, st = sc.render(tree, None, spp=4, guided=False, seed=606)
    a = a.clone()
    monkeypatch.setenv("SDMM_MESH_BRUTE", "1")
    brute = pkg.Scene(desc)
    monkeypatch.delenv("SDMM_MESH_BRUTE")
    b, _, sb = brute.render(tree, None, spp=4, guided=False, seed=606)
    assert torch.equal(a, b) and st == sb and np.isfinite(a.cpu().numpy()).all() and float(a.mean()) > 0
    one = pkg.Scene(scenes.sheet_scene(64, 36, twosided=False))
    c = one.render(tree, None, spp=4, guided=False, seed=606)[0]
    assert not torch.equal(a, c)
