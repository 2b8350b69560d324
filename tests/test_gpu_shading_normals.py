"""GPU: vertex normals on meshes in the device Li (sdmm_scene_desc.mesh_normals,
sdmm_li_params.non_strict_normals; csrc/shading_normal.h).  The CPU oracle's Li
knows face normals only, so the yardsticks are the host entry (itself pinned to
a numpy restatement in tests/test_shading_cases.py), exact constructions and
analytic values:

  1. Scene.shading equals shading_host bitwise, at every batch size and mode;
  2. exact inertness: axis-aligned triangles whose vertex normals are the exact
     axis vectors render, record and train bitwise as without normals -- the
     NRM kernel variants against the others, path by path;
  3. a flat one-sided diffuse sheet whose vertex normals are tilted by 60
     degrees under a constant sky: rho L everywhere without strictNormals; with
     them a quarter of the paths end ((1 - cos 60) / 2 of the clamped-cosine
     lobe lies below the sheet), exactly those without a vertex;
  4. the saved normals on the smooth torus are the interpolated normals at the
     saved positions;
  5. the mirror twin with normals: a torus probe met from behind in the
     mirrored scene gives bitwise the mirrored image and records;
  6. guided and product renders of torus_scene(smooth_normals=True) agree with
     the BSDF-only one on the mean, the producer equals the oracle;
  7. the BVH image is the brute loop's, with normals;
  8. a two-sided sheet with smooth normals saves -ns behind.
"""
import numpy as np
import pytest

import mesh_fixture as mf
import shading_cases as sc
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
    return rec.reshape(16, V, -1).copy(), nv.copy(), V


# ---- 1: the device entry against the host entry ------------------------------------------------
@pytest.mark.parametrize("name", ["torus_benign", "torus_hard", "flip", "vanish"])
def test_scene_shading_equals_host(pkg, scenes, gpu, name):
    import torch
    desc, o, d = sc.cases(scenes)[name]
    scene = pkg.Scene(mf.camera_fields(desc))
    sizes = [n for n in (1, 63, 64, 65, 257, 4099) if n <= len(o)] + ([len(o)] if len(o) < 4099 else [])
    for mode in (0, 1):
        want = pkg.shading_host(desc, o, d, mint=mf.MINT, mode=mode)
        for n in sizes:
            ot = [torch.from_numpy(o[:n, a].copy()).to(gpu) for a in range(3)]
            dt = [torch.from_numpy(d[:n, a].copy()).to(gpu) for a in range(3)]
            prim, t, ns, ng = scene.shading(ot, dt, mint=mf.MINT, mode=mode)
            torch.cuda.synchronize()
            assert np.array_equal(prim.cpu().numpy(), want[0][:n]), (name, mode, n)
            assert np.array_equal(_bits(t.cpu().numpy()), _bits(want[1][:n])), (name, mode, n)
            got_ns = np.stack([x.cpu().numpy() for x in ns], 1)
            got_ng = np.stack([x.cpu().numpy() for x in ng], 1)
            assert np.array_equal(_bits(got_ns), _bits(want[2][:n])), (name, mode, n)
            assert np.array_equal(_bits(got_ng), _bits(want[3][:n])), (name, mode, n)
    # and sdmm_scene_intersect's (prim, t) are this entry's
    p0, t0 = scene.intersect(ot, dt, mint=mf.MINT)
    assert torch.equal(p0, prim) and np.array_equal(_bits(t0.cpu().numpy()), _bits(t.cpu().numpy()))


# ---- 2: exact inertness ----------------------------------------------------------------------
def _axis_room(scenes, w, h, normals):
    """A room (inward faces), a block in it and an emitting patch under the
    ceiling, all axis-aligned and all triangles: every face owns its four
    vertices, whose normals are the face's exact axis unit vector."""
    quads, bsdf, emit = [], [], []

    def box(lo, hi, inward, b):
        lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
        M = np.zeros((3, 4))
        M[:, :3] = np.diag(0.5 * (hi - lo))
        M[:, 3] = 0.5 * (hi + lo)
        for p0, e1, e2 in scenes._cube_faces(M):
            quads.append(np.concatenate((p0, e2, e1) if inward else (p0, e1, e2)))
            bsdf.append(b); emit.append(-1)
    box((-2.0, 0.0, -2.0), (2.0, 3.0, 2.0), True, 0)
    box((-0.75, 0.0, -0.5), (0.25, 1.25, 0.5), False, 1)
    quads.append(np.array([-0.5, 2.875, -0.5, 1.0, 0, 0, 0, 0, 1.0]))        # e1 x e2 = -y: the lamp faces down
    bsdf.append(2); emit.append(0)
    q = np.asarray(quads, np.float32)
    verts, tris = scenes.quads_to_triangles(q)
    qn = np.cross(q[:, 3:6].astype(np.float64), q[:, 6:9].astype(np.float64))
    qn = np.sign(qn) * (np.abs(qn) > 0)                                   # exactly (+-1, 0, 0) and so on
    assert (np.abs(qn).sum(1) == 1).all()
    d = {"reflectance": np.asarray([0.7, 0.65, 0.6, 0.3, 0.6, 0.8, 0, 0, 0], np.float32),
         "mesh_vertices": verts.reshape(-1), "triangles": tris.reshape(-1),
         "tri_bsdf": np.repeat(np.asarray(bsdf, np.int32), 2), "tri_emitter": np.repeat(np.asarray(emit, np.int32), 2),
         "radiance": np.asarray([14.0, 12.0, 9.0], np.float32),
         "camera_to_world": scenes._look_at((1.3, 1.7, 1.8), (-0.3, 0.8, 0.0), (0.0, 1.0, 0.0)),
         "fov_x_deg": 60.0, "near_clip": 1e-2, "width": w, "height": h}
    if normals:
        d["mesh_normals"] = np.repeat(qn, 4, axis=0).astype(np.float32).reshape(-1) + np.float32(0.0)   # (no -0)
    return d


def test_exact_axis_normals_are_inert(pkg, scenes, gpu):
    import torch
    W, H = 64, 36
    plain, smooth = pkg.Scene(_axis_room(scenes, W, H, False)), pkg.Scene(_axis_room(scenes, W, H, True))
    tree = _tree(pkg, plain)
    node_mix = _train(pkg, plain, tree, 2, 8, K=16)
    assert any(m is not None for m in node_mix)
    for guided in (False, True):
        kw = dict(spp=2, guided=guided, seed=51 + guided)
        a, va, sa = plain.render(tree, node_mix if guided else None, **kw)
        a = a.clone()
        ra, na, V = _saved(va)
        b, vb, sb = smooth.render(tree, node_mix if guided else None, **kw)
        rb, nb, _ = _saved(vb)
        assert torch.equal(a, b) and sa == sb and np.array_equal(na, nb)       # (== on floats: a zero of either sign is equal)
        assert na.sum() > W * H and float(a.mean()) > 0 and (not guided or sa["guided_queries"] > 0)
        sel = np.arange(V)[:, None] < na[None, :]
        for f in range(16):
            assert np.array_equal(ra[f][sel], rb[f][sel]), f


# ---- 3: the tilted flat sheet -------------------------------------------------------------------
TILT = np.radians(60.0)


def _tilted_sheet(scenes, w, h):
    d = tf.flat_sheet(scenes, False, w, h)                 # one-sided; one cell's winding faces down
    ns = np.asarray([0.0, np.cos(TILT), np.sin(TILT)], np.float32)
    d["mesh_normals"] = np.tile(ns, 6)
    return d, ns.astype(np.float64) / np.linalg.norm(ns.astype(np.float64))


def test_tilted_sheet_strict_and_not(pkg, scenes, gpu, plog):
    W, H = 64, 36
    desc, ns = _tilted_sheet(scenes, W, H)
    scene = pkg.Scene(desc)
    tree = _tree(pkg, scene)
    want = np.float32(tf.SHEET_RHO) * np.float32(tf.SHEET_L)
    o, d = tf.camera_rays(desc)
    on = pkg.shading_host(desc, o, d)[0] >= 0
    out = {}
    for strict in (False, True):
        img, verts, st = scene.render(tree, None, spp=1, max_depth=3, guided=False, seed=66, strict_normals=strict)
        r, nv, V = _saved(verts)
        out[strict] = (img.cpu().numpy().reshape(3, -1).copy(), r, nv)
    img, r, nv = out[False]
    hit = nv == 1
    assert hit.sum() > 400 and (nv <= 1).all() and hit[on].mean() > 0.9
    rel = np.abs(img[:, hit].astype(np.float64) - want[:, None]) / want[:, None]
    print(f"tilted sheet, not strict: {int(hit.sum())} sheet pixels, largest relative error {rel.max():.3g}")
    assert rel.max() <= 1e-6
    assert np.array_equal(img[:, ~hit], np.broadcast_to(np.float32(tf.SHEET_L)[:, None], (3, int((~hit).sum()))))
    # the saved normal is the tilted one, not the face normal (0, +-1, 0)
    saved = np.stack([r[13 + a][0][hit] for a in range(3)], 1).astype(np.float64)
    assert np.abs(saved - ns).max() <= 1e-6 and abs(ns[1] - 1.0) > 0.4
    # some directions sampled about ns dip below the sheet: only the non-strict render follows them
    wo_y = r[11][0][hit]
    assert (wo_y < 0).mean() > 0.15
    simg, sr, snv = out[True]
    sheet = hit                                                       # the same camera rays meet the sheet
    zero = sheet & (simg.max(0) == 0)
    alive = sheet & ~zero
    assert np.array_equal(zero, sheet & (snv == 0)) and np.array_equal(alive, snv == 1)
    rel = np.abs(simg[:, alive].astype(np.float64) - want[:, None]) / want[:, None]
    assert rel.max() <= 1e-6 and (simg[:, zero] == 0).all()
    assert (sr[11][0][alive] > 0).all()                               # wo . ng > 0, ng = (0, 1, 0) on both cells
    # the survivors are the non-strict render's paths, bit for bit; the others are those that went below
    assert np.array_equal(_bits(simg[:, alive]), _bits(img[:, alive])) and np.array_equal(zero, sheet & (wo_y_full(r, hit) <= 0))
    N = int(sheet.sum())
    share, expect = zero.sum() / N, (1.0 - np.cos(TILT)) / 2.0
    sd = np.sqrt(expect * (1.0 - expect) / N)
    plog("tilted_sheet_strict_zero_share_sigma", abs(share - expect) / sd, 4.0, share=float(share), paths=N)
    print(f"tilted sheet, strict: {int(zero.sum())} of {N} paths end ({share:.4f}, expected {expect:.4f}, sd {sd:.4f})")
    assert abs(share - expect) <= 4.0 * sd


def wo_y_full(r, hit):
    y = np.full(hit.shape, np.inf, np.float32)
    y[hit] = r[11][0][hit]
    return y


# ---- 4: saved normals on the smooth torus ---------------------------------------------------------
def test_saved_normals_are_the_interpolated_ones(pkg, scenes, gpu, plog):
    desc = mf.camera_fields(sc.torus_desc(scenes), 64, 36)
    scene = pkg.Scene(desc)
    img, verts, st = scene.render(_tree(pkg, scene), None, spp=2, max_depth=2, guided=False, seed=12)
    r, nv, V = _saved(verts)
    smin, snorm, _, _ = scene.normalization()
    p, _, n = tf.vertex_table(r.reshape(-1), nv, V, smin, snorm)
    assert len(p) > 1500 and (nv <= 1).all()
    cam = np.asarray(desc["camera_to_world"], np.float64).reshape(4, 4)[:3, 3]
    o = np.broadcast_to(cam, p.shape)
    d = p - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    prim, t, ns, ng = pkg.shading_host(desc, o, d, mint=0.0)
    hit = prim >= 0
    assert (~hit).mean() <= 1e-3
    on_torus = hit & (prim >= 3)
    assert on_torus.sum() > 500
    dev = np.abs(n[hit].astype(np.float64) - ns[hit]).max(1)
    face = np.abs(n[on_torus].astype(np.float64) - ng[on_torus]).max(1)
    plog("saved_normal_vs_interpolated_max_abs", dev.max(), 1e-4, vertices=int(hit.sum()), missed=int((~hit).sum()))
    print(f"saved normals: {int(hit.sum())} vertices, largest deviation from ns {dev.max():.3g}; "
          f"from the face normal up to {face.max():.3g}")
    assert dev.max() <= 1e-4 and face.max() > 0.1


# ---- 5: the mirror twin with normals ----------------------------------------------------------------
def _torus_twin(scenes, kind, w, h):
    """(A, B): the emitting cube of twosided_fixture.twin_scenes round a torus
    probe with its analytic vertex normals; B = mirror_z(A, keep = the torus):
    B's shading normals are -mirror(ns), so what meets A's probe from the front
    meets B's from behind.  The probe's BSDF is two-sided in both: a grazing
    bounce ray can meet its own triangle again from the other side (one path in
    some thousands does), which is then a back hit in A and a front hit in B --
    mirrored too, where a one-sided A would end the path."""
    cube = np.array([[3.0, 0, 0, 0], [0, 3.0, 0, 0], [0, 0, 3.0, 0]])
    quads = [np.concatenate(f) for f in scenes._cube_faces(cube)]
    bp, refl = tf.probe_material(scenes, kind)
    T = np.array([[1.0, 0, 0, 0.05], [0, 0.6, -0.8, 0.0], [0, 0.8, 0.6, 0.1]])       # tilted: no axis of symmetry in z = 0
    v, t, n = scenes.torus_mesh(24, 12, 1.0, 0.4, to_world=T, normals=True)
    A = {"quads": np.asarray(quads, np.float32).reshape(-1), "flip_normals": np.ones(6, np.int32),
         "bsdf": np.zeros(6, np.int32), "reflectance": np.concatenate([np.zeros(3, np.float32), refl]).astype(np.float32),
         "emitter": np.arange(6, dtype=np.int32), "radiance": tf.FACE_RADIANCE.reshape(-1).copy(),
         "mesh_vertices": v.reshape(-1), "triangles": t.reshape(-1), "tri_bsdf": np.ones(len(t), np.int32),
         "mesh_normals": n.reshape(-1),
         "camera_to_world": tf._look_from((0.37, 0.53, 2.6), (0.05, -0.07, 0.0)), "fov_x_deg": 50.0, "near_clip": 1e-2,
         "width": w, "height": h, "bsdf_params": np.concatenate([np.zeros(8, np.float32), bp]).astype(np.float32)}
    A["bsdf_twosided"] = np.asarray([0, 1], np.int32)
    B = scenes.mirror_z(A, keep=tuple(6 + np.arange(len(t))))
    assert B["tri_flip_normals"].all() and not B["flip_normals"].any()
    return A, B


def _torus_twin_check(pkg, scenes, kind, w, h, pixels, seed):
    A, B = _torus_twin(scenes, kind, w, h)
    out = []
    for desc in (A, B):
        scene = pkg.Scene(desc)
        img, verts, st = scene.render(_tree(pkg, scene), None, spp=1, max_depth=3, guided=False, seed=seed, pixels=pixels)
        r, nv, V = _saved(verts)
        out.append((img.cpu().numpy().copy(), r, nv, st))
    (ia, ra, na, sa), (ib, rb, nb, sb) = out
    n_paths = w * h if pixels is None else pixels[1] - pixels[0]
    assert sa["paths"] == n_paths and sa == sb, (sa, sb)
    assert np.array_equal(na, nb)
    assert np.array_equal(_bits(ia), _bits(ib))
    assert (ia.reshape(3, -1).max(0) > 0).sum() > 0.6 * n_paths        # (pixels outside `pixels` stay 0)
    V = ra.shape[1]
    sel = np.arange(V)[:, None] < na[None, :]
    for f in range(16):
        a, b = ra[f][sel], rb[f][sel]
        if f == 9:
            # c.z = (p.z - scene_min.z) / norm over the symmetric box: c.z and 1 - c.z, each rounded
            assert np.abs(a.astype(np.float64) + b - 1.0).max(initial=0.0) <= 1e-6
        elif f in (12, 15):
            assert np.array_equal(_bits(a), _bits(-b)), f
        else:
            assert np.array_equal(_bits(a), _bits(b)), f
    return ra, na, sa, sel


@pytest.mark.parametrize("kind", [0, 3, 6])
def test_mirror_twin_with_normals(pkg, scenes, gpu, kind):
    W = H = 32
    ra, nv, st, sel = _torus_twin_check(pkg, scenes, kind, W, H, None, 700 + kind)
    if kind == 6:
        assert (nv == 0).all() and st["segments"] > 0.4 * W * H           # delta only: no vertex, the rays still traced
    else:
        assert (nv >= 1).sum() > 0.4 * W * H
        # the probe's saved normals are smooth ones: not one of the 576 face normals repeats
        n = np.stack([ra[13 + a][0][nv >= 1] for a in range(3)], 1)
        assert len(np.unique(n, axis=0)) > 0.9 * len(n)


def test_mirror_twin_with_normals_across_blocks(pkg, scenes, gpu):
    """4099 paths of the Phong twin: more than sixteen 256-thread blocks and a tail."""
    _, nv, _, _ = _torus_twin_check(pkg, scenes, 3, 128, 64, (5, 5 + 4099), 78)
    assert len(nv) == 4099 and (nv >= 1).sum() > 1500


# ---- 6: guided and product renders of the smooth torus scene -------------------------------------------
SW, SH = 48, 27


def test_smooth_torus_guided_and_product_unbiased(pkg, oracle, scenes, gpu, plog):
    import torch
    desc = scenes.torus_scene(SW, SH, nu=24, nv=12, smooth_normals=True)
    assert "mesh_normals" in desc
    scene = pkg.Scene(desc)
    tree = _tree(pkg, scene)
    node_mix = _train(pkg, scene, tree, 4, 8, K=16)
    assert any(m is not None for m in node_mix)
    B = len(desc["reflectance"]) // 3
    w, m, cov, dif = scenes.diffuse_learned_bsdf(B)
    table = pkg.BsdfTable(w, m, cov, device=gpu, diffuse=dif)
    for tag, kw in (("smooth_torus_guided", {}), ("smooth_torus_product", {"learned_bsdf": table})):
        img, verts, st = scene.render(tree, node_mix, spp=4, guided=True, seed=77, **kw)
        assert np.isfinite(img.cpu().numpy()).all() and st["guided_queries"] > 0
        _check_producer(pkg, oracle, tree, verts, 8, 0xAD0, plog, tag)
    spp = 64
    u_img = scene.render(tree, None, spp=spp, guided=False, seed=4330)[0].clone()
    u = _lum(u_img)
    for what, kw, seed in (("guided", {}, 2360), ("product", {"learned_bsdf": table}, 2361)):
        g = _lum(scene.render(tree, node_mix, spp=spp, guided=True, seed=seed, **kw)[0])
        assert np.isfinite(g).all()
        s = plog(f"li_smooth_torus_{what}_vs_unguided_mean_sigma", _sigma(g, u), 4.0, guided=float(g.mean()),
                 unguided=float(u.mean()))
        print(f"smooth torus {what}: mean {g.mean():.5f} against BSDF-only {u.mean():.5f} ({s:.2f} sigma)")
        assert s < 4.0, (what, g.mean(), u.mean())
    faceted = pkg.Scene(scenes.torus_scene(SW, SH, nu=24, nv=12))
    f_img = faceted.render(tree, None, spp=spp, guided=False, seed=4330)[0]
    assert not torch.equal(u_img, f_img)


# ---- 7: BVH == brute ---------------------------------------------------------------------------------
def test_smooth_bvh_equals_brute(pkg, scenes, gpu, monkeypatch):
    import torch
    monkeypatch.delenv("SDMM_MESH_BRUTE", raising=False)
    desc = scenes.torus_scene(64, 36, nu=24, nv=12, smooth_normals=True)
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


# ---- 8: a two-sided sheet with smooth normals ----------------------------------------------------------
def test_twosided_smooth_sheet_saves_negated_normals(pkg, scenes, gpu, plog):
    desc = scenes.sheet_scene(SW, SH, smooth_normals=True)
    assert "mesh_normals" in desc and desc["bsdf_twosided"][int(desc["tri_bsdf"][0])] == 1
    scene = pkg.Scene(desc)
    img, verts, st = scene.render(_tree(pkg, scene), None, spp=4, guided=False, seed=77)
    assert np.isfinite(img.cpu().numpy()).all()
    r, nv, V = _saved(verts)
    smin, snorm, _, _ = scene.normalization()
    p, _, n = tf.vertex_table(r.reshape(-1), nv, V, smin, snorm)
    on = tf.on_sheet(desc, p)
    assert on.sum() > 1000
    # the interpolated normal at each such vertex: a short ray straight down onto it (the sheet is a height field)
    o = p[on] + np.asarray([0.0, 0.05, 0.0])
    d = np.broadcast_to(np.asarray([0.0, -1.0, 0.0]), o.shape)
    prim, t, ns, ng = pkg.shading_host(desc, o, d, mint=0.0)
    nq = len(desc["quads"]) // 9
    ok = prim >= nq
    assert ok.mean() > 0.99 and (ns[ok, 1] > 0).all()                    # the analytic normals are on the +y side
    got = n[on][ok].astype(np.float64)
    front = np.abs(got - ns[ok]).max(1)
    back = np.abs(got + ns[ok]).max(1)
    dev = np.minimum(front, back)
    negated = back < front
    share = float(negated.mean())
    plog("smooth_sheet_back_vertex_share", share, 0.30, lower=True, sheet_vertices=int(ok.sum()))
    plog("smooth_sheet_saved_normal_vs_pm_ns_max_abs", dev.max(), 1e-4)
    print(f"smooth two-sided sheet: {int(ok.sum())} vertices, {share:.3f} of them save -ns; largest deviation {dev.max():.3g}")
    assert dev.max() <= 1e-4 and share >= 0.30
    assert np.array_equal(negated, got[:, 1] < 0)
    # and they are not the face normals
    assert np.minimum(np.abs(got - ng[ok]).max(1), np.abs(got + ng[ok]).max(1)).max() > 0.02
