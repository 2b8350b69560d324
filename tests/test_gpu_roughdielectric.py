"""GPU: the rough dielectric in the device Li (bsdf kind 4,
csrc/bsdf_roughdielectric.h): the batch kernel behind
sdmm_bsdf_roughdielectric_device equals the host call bitwise; a furnace (a
pane inside a box of unit emitters) renders the BSDF's float64 albedo from
either side, BSDF-only, guided and with the product; a glass box in the
Cornell Box is unbiased against its BSDF-only render, trains bitwise like the
host-routed oracle and saves inward normals inside the glass; Russian roulette
with the relative index leaves the mean unchanged.

The dielectric bounce is compared path by path with the CPU Li oracle in
tests/test_gpu_li_oracle_dielectric.py (the oracle's own restatement of the
material is pinned in tests/test_li_oracle_dielectric.py)."""
import numpy as np
import pytest

from test_bsdf_roughdielectric import ETA, HostBsdf, albedo64, params, sphere_wi
from test_gpu_li import _check_producer, _train, _tree

pytestmark = pytest.mark.gpu

ALPHA = 0.3


# ---- batch kernel == host --------------------------------------------------
def _host_F(host, wi, u0, u1):
    """The library's float32 F at the microfacet normal of (u0, u1): the
    largest float u2 whose sample reflects, by bisection over the bit patterns
    (None: no transmitted lobe to tell it by)."""
    def reflects(bits):
        u2 = np.uint32(bits).view(np.float32)
        _, _, _, eta = host.sample(wi, (u0, u1, u2))
        return eta == 1.0
    hi = int(np.float32(1.0).view(np.uint32)) - 1          # the largest float below 1
    if not reflects(0) or reflects(hi):
        return None
    lo = 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if reflects(mid) else (lo, mid)
    return np.uint32(lo).view(np.float32)


def edge_rows(pkg, scenes):
    """The batch test's inputs: (rng, bp, st, host, W, U) -- 4099 rows of wi
    over the whole sphere and uniforms with the edges placed by hand: wi.z of
    0 and +-1e-4, inside hits beyond the critical angle, u0 of 0 and of the
    largest float below 1, u2 == F and the next float above it."""
    rng = np.random.default_rng(4099)
    nq = 4099                                              # a tail in the last workgroup
    bp, st = params(scenes, 0.2, (0.9, 0.8, 0.7), (0.6, 0.95, 0.85))
    host = HostBsdf(pkg, bp, st)
    W = sphere_wi(rng, nq, 0.0)
    U = rng.uniform(0, 1, (nq, 3)).astype(np.float32)
    below1 = np.float32(1 - 2.0 ** -24)
    W[0] = (0.6, 0.8, 0.0)                                 # wi.z = 0 exactly
    W[1] = (0.6, 0.8, 1e-4)
    W[2] = (0.6, 0.8, -1e-4)
    for i in range(3, 40):                                 # inside, beyond the critical angle (sin > 1 / eta)
        s = rng.uniform(0.7, 0.999)
        W[i] = (s, 0.0, -np.sqrt(1 - s * s))
    U[40:60, 0] = 0.0
    U[60:80, 0] = below1
    U[80:90, 2] = below1
    n_tie = 0
    for i in range(100, 140):                              # u2 == F exactly, and the next float above it
        F = _host_F(host, W[i], U[i, 0], U[i, 1])
        if F is not None:
            U[i, 2] = F if i % 2 == 0 else np.nextafter(F, np.float32(2))
            n_tie += 1
    assert n_tie > 10 and (W[:, 2] < 0).sum() > 1500 and (W[:, 2] > 0).sum() > 1500
    return rng, bp, st, host, W, U


def test_batch_kernel_equals_host_bitwise(pkg, scenes, gpu):
    import torch
    rng, bp, st, host, W, U = edge_rows(pkg, scenes)
    nq = len(W)
    dev = lambda a: [torch.from_numpy(np.ascontiguousarray(a[:, i])).to(gpu) for i in range(3)]
    wo_d, val_d, pdf_d, eta_d = pkg.bsdf_roughdielectric_device(bp, st, dev(W), u=dev(U))
    torch.cuda.synchronize()
    got = np.stack([t.cpu().numpy() for t in wo_d + val_d + [pdf_d, eta_d]], 1)
    ref = np.float32([np.concatenate([(r := host.sample(w, u))[0], r[1], [r[2], r[3]]]) for w, u in zip(W, U)])
    mism = int((got.view(np.uint32) != ref.view(np.uint32)).any(1).sum())
    print(f"roughdielectric batch sample: {mism} of {nq} rows differ from the host call; "
          f"{int((ref[:, 6] == 0).sum())} void, {int((ref[:, 7] != 1).sum())} transmitted")
    assert mism == 0
    assert (ref[:, 6] == 0).sum() > 50 and (ref[:, 7] == np.float32(bp[4])).sum() > 500
    assert (ref[:, 7] == np.float32(bp[5])).sum() > 300
    # the ties: reflection at u2 == F, transmission just above
    for i in range(100, 140):
        if U[i, 2] != 0 and _host_F(host, W[i], U[i, 0], U[i, 1]) is not None:
            assert (ref[i, 7] == 1.0) == (i % 2 == 0)
    # eval mode: the sampled directions, independent ones on a third, wo.z = 0
    WO = ref[:, :3].copy()
    WO[::3] = sphere_wi(rng, len(WO[::3]), 0.0)
    WO[5] = (0.0, 1.0, 0.0)
    _, val_e, pdf_e, eta_e = pkg.bsdf_roughdielectric_device(bp, st, dev(W), wo=dev(WO))
    torch.cuda.synchronize()
    got = np.stack([t.cpu().numpy() for t in val_e + [pdf_e, eta_e]], 1)
    ref_e = np.float32([np.concatenate([(r := host.eval(w, o))[0], [r[1], r[2]]]) for w, o in zip(W, WO)])
    mism = int((got.view(np.uint32) != ref_e.view(np.uint32)).any(1).sum())
    print(f"roughdielectric batch eval: {mism} of {nq} rows differ; {int((ref_e[:, 3] > 0).sum())} with pdf > 0")
    assert mism == 0 and (ref_e[:, 3] > 0).sum() > 2000 and (ref_e[0, :4] == 0).all()


# ---- furnace -----------------------------------------------------------------
FW, FH, INC = 64, 36, 50.0


def _furnace(scenes, R, T, flip=False, model=None, second_pane=False):
    """A box [-3, 3]^3 of six inward-facing emitters of radiance 1 (zero
    reflectance), a free-standing kind-4 pane z = 0 of side 4 in it (normal
    +z, -z with flip), the camera inside at 2 (sin INC, 0, cos INC) looking at
    the origin with a 4 degree field of view -- 0.2 degrees from behind, where
    50 degrees lies beyond the critical angle and the albedo changes by 2 per
    radian: a wider pixel's corners would leave its centre's albedo by more
    than a quarter of the standard error.  second_pane: another pane at z = -1
    (paths of several bounces)."""
    cube = np.array([[3.0, 0, 0, 0], [0, 3.0, 0, 0], [0, 0, 3.0, 0]])
    quads = [np.concatenate(f) for f in scenes._cube_faces(cube)]
    bsdf, flips, emitter = [0] * 6, [1] * 6, [0] * 6
    for z in ([0.0, -1.0] if second_pane else [0.0]):
        quads.append(np.array([-2.0, -2.0, z, 4.0, 0, 0, 0, 4.0, 0]))
        bsdf.append(1); flips.append(int(flip)); emitter.append(-1)
    bp = np.zeros((2, 8), np.float32)
    bp[1], tr = params(scenes, ALPHA, (R,) * 3, (T,) * 3)
    inc = np.radians(INC)
    pos = 2.0 * np.array([np.sin(inc), 0.0, np.cos(inc)])
    fwd = -pos / np.linalg.norm(pos)
    right = np.cross([0.0, 1.0, 0.0], fwd)
    right /= np.linalg.norm(right)
    up = np.cross(fwd, right)
    cam = np.concatenate([np.stack([right, up, fwd, pos], 1).reshape(-1), [0, 0, 0, 1]]).astype(np.float32)
    desc = {"quads": np.asarray(quads, np.float32).reshape(-1), "flip_normals": np.asarray(flips, np.int32),
            "bsdf": np.asarray(bsdf, np.int32), "reflectance": np.concatenate([np.zeros(3), tr]).astype(np.float32),
            "emitter": np.asarray(emitter, np.int32), "radiance": np.ones(3, np.float32), "camera_to_world": cam,
            "fov_x_deg": 0.2 if flip else 4.0, "near_clip": 1e-2, "width": FW, "height": FH,
            "bsdf_params": bp.reshape(-1)}
    if model is not None:
        desc["learned_models_nd"] = [None, model]
    return desc


def _pixel_cos(desc, corners=False):
    """cos theta_i on the pane at the pixel centres (or the four corners) of
    the camera kernel's perspective mapping, float64."""
    cam = desc["camera_to_world"].astype(np.float64).reshape(4, 4)[:3]
    tanx = np.tan(0.5 * np.radians(desc["fov_x_deg"]))
    offs = [(0.5, 0.5)] if not corners else [(0, 0), (0, 1), (1, 0), (1, 1)]
    out = []
    for ox, oy in offs:
        sx = (np.arange(FW) + ox) / FW
        sy = (np.arange(FH) + oy) / FH
        SX, SY = np.meshgrid(sx, sy)
        l = np.stack([(1 - 2 * SX) * tanx, (1 - 2 * SY) * tanx / (FW / FH), np.ones_like(SX)], -1)
        d = l @ cam[:, :3].T
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
        out.append(np.abs(d[..., 2]))
    return np.stack(out)


_ALBEDO = {}
SE_MIN = 1.5e-4          # below every render's standard error here (>= 2e-4 at 64 x 36 x 256 samples)


def _albedo_fit(scenes, R, T, side, se):
    """The float64 albedo (tests/test_bsdf_roughdielectric.py albedo64, each
    quadrature refined until it changes by less than se / 4) as a polynomial
    in cos theta_i over the view's range: 5 quadratures, degree 2; the fit's
    residual at the nodes must be below se / 8."""
    key = (R, T, side)
    if key not in _ALBEDO:
        desc = _furnace(scenes, R, T, side < 0)
        c = _pixel_cos(desc, corners=True)
        nodes = np.linspace(c.min(), c.max(), 5)
        bp, _ = params(scenes, ALPHA)
        vals = [albedo64(side * x, float(bp[4]), ALPHA, (R,) * 3, (T,) * 3, se)[0] for x in nodes]
        poly = np.polynomial.Polynomial.fit(nodes, vals, 2)
        assert np.max(np.abs(poly(nodes) - vals)) < se / 8
        _ALBEDO[key] = poly
    return _ALBEDO[key]


def _known_answer(scenes, desc, R, T, side, img, what, plog):
    """The mean over the pixels (every ray meets the pane) against the albedo
    at the pixel centres, averaged, within 4 standard errors."""
    px = img.cpu().numpy()[0].astype(np.float64)
    assert np.isfinite(px).all()
    se = float(px.std(ddof=1) / np.sqrt(px.size))
    assert se >= SE_MIN                                     # the quadrature was refined for that
    poly = _albedo_fit(scenes, R, T, side, SE_MIN)
    centre = poly(_pixel_cos(desc)[0])
    corner_gap = float(np.max(np.abs(poly(_pixel_cos(desc, corners=True)) - centre[None])))
    assert corner_gap < 0.25 * se, (corner_gap, se)         # else: narrow the view
    ref = float(centre.mean())
    s = abs(px.mean() - ref) / se
    plog(f"furnace_{what}_sigma", s, 4.0, mean=float(px.mean()), albedo=ref, se=se)
    print(f"furnace {what}: mean {px.mean():.5f} +- {se:.5f}, albedo {ref:.5f} ({s:.2f} sigma), corner gap "
          f"{corner_gap:.2g}")
    assert se > 0 and s < 4.0, (what, px.mean(), ref, se)


@pytest.mark.parametrize("R,T,flip", [(1.0, 1.0, False), (1.0, 1.0, True), (1.0, 0.0, False), (0.0, 1.0, False),
                                      (0.0, 1.0, True)])
def test_furnace_bsdf_only(pkg, scenes, gpu, plog, R, T, flip):
    desc = _furnace(scenes, R, T, flip)
    sc = pkg.Scene(desc)
    tree = _tree(pkg, sc)
    img, verts, st = sc.render(tree, None, spp=256, guided=False, seed=1301)
    _known_answer(scenes, desc, R, T, -1.0 if flip else 1.0, img, f"bsdf_R{R:g}_T{T:g}_{'back' if flip else 'front'}",
                  plog)
    rec, nv = verts.to_numpy()
    V = verts.s.max_vertices
    n = rec.reshape(16, V, -1)[13:16, 0][:, nv > 0]
    # the saved vertex carries the normal of the side the path came from
    assert (n[2] == 1.0).all() and (n[0] == 0).all()


def _below_share(verts):
    """Of the first saved vertices (all on the pane), the share whose saved
    direction lies below the saved normal."""
    rec, nv = verts.to_numpy()
    r = rec.reshape(16, verts.s.max_vertices, -1)[:, 0][:, nv > 0]
    return float(np.mean((r[10:13] * r[13:16]).sum(0) < 0))


@pytest.mark.parametrize("flip", [False, True])
def test_furnace_guided_and_product(pkg, scenes, gpu, plog, flip):
    """The shade kernel's transmitted eval / pdf without a second copy of the
    same code: guided (plain conditional) and product renders (with the
    shipped model and with none) give the float64 albedo."""
    model = scenes.load_learned_nd(scenes.LEARNED_DIELECTRIC)
    side = -1.0 if flip else 1.0
    desc = _furnace(scenes, 1.0, 1.0, flip, model=model)
    sc = pkg.Scene(desc)
    bare = pkg.Scene(_furnace(scenes, 1.0, 1.0, flip))
    tree = _tree(pkg, sc)
    node_mix = _train(pkg, sc, tree, 4, 8, K=16)
    assert any(m is not None for m in node_mix)
    w, m, cov, dif = scenes.diffuse_learned_bsdf(2)
    table = pkg.BsdfTable(w, m, cov, device=gpu, diffuse=dif)
    tag = "back" if flip else "front"
    for what, scene, kw in (("guided", sc, {}), ("product_model", sc, {"learned_bsdf": table}),
                            ("product_nomodel", bare, {"learned_bsdf": table})):
        img, verts, st = scene.render(tree, node_mix, spp=256, guided=True, seed=1402, **kw)
        below = _below_share(verts)
        print(f"furnace {what} {tag}: guided_queries {st['guided_queries']}, saved directions below the pane "
              f"{100 * below:.1f} %")
        assert st["guided_queries"] > 0 and below >= 0.10, "vacuous"
        _known_answer(scenes, desc, 1.0, 1.0, side, img, f"{what}_{tag}", plog)


def test_furnace_russian_roulette(pkg, scenes, gpu, plog):
    """rr_depth = 1 in a furnace with two panes (paths of several bounces, the
    relative index leaving 1): the BSDF-only mean is unchanged within 4 sigma.
    Roulette is unbiased for any survival probability, so this guards against
    a bad eta plane (NaN, zero), not against a wrong value."""
    desc = _furnace(scenes, 1.0, 1.0, second_pane=True)
    sc = pkg.Scene(desc)
    tree = _tree(pkg, sc)
    a = sc.render(tree, None, spp=256, guided=False, seed=1501, rr_depth=1)[0].cpu().numpy()[0].astype(np.float64)
    b = sc.render(tree, None, spp=256, guided=False, seed=1502, rr_depth=10)[0].cpu().numpy()[0].astype(np.float64)
    assert np.isfinite(a).all() and np.isfinite(b).all()
    se = np.sqrt(a.var(ddof=1) / a.size + b.var(ddof=1) / b.size)
    s = plog("furnace_rr1_vs_rr10_sigma", abs(a.mean() - b.mean()) / se, 4.0, rr1=float(a.mean()), rr10=float(b.mean()))
    assert s < 4.0, (a.mean(), b.mean())
    # one pane, where the bounce after it only meets an emitter: the known answer itself
    one = _furnace(scenes, 1.0, 1.0)
    img = pkg.Scene(one).render(tree, None, spp=256, guided=False, seed=1503, rr_depth=1)[0]
    _known_answer(scenes, one, 1.0, 1.0, 1.0, img, "bsdf_rr1_front", plog)


# ---- Cornell glass box -----------------------------------------------------------
GLASS = ("TallBox",)
LIFT = 0.02


def _lum(im):
    return im.cpu().numpy().mean(0).reshape(-1)


def _sigma(a, b):
    se = np.sqrt(a.var() / a.size + b.var() / b.size)
    return float(abs(a.mean() - b.mean()) / se)


def _inside_inward(scenes, sc, verts):
    """Saved vertices on a face of the lifted TallBox that carry the inward
    normal (a step along it leads strictly into the box), per path."""
    rec, nv = verts.to_numpy()
    V = verts.s.max_vertices
    r = rec.reshape(16, V, -1)
    sel = np.arange(V)[:, None] < nv[None, :]
    smin, snorm, _, _ = sc.normalization()
    p = np.stack([r[7 + a][sel] for a in range(3)], 1).astype(np.float64) * snorm + smin
    n = np.stack([r[13 + a][sel] for a in range(3)], 1).astype(np.float64)
    M = scenes._mat(dict((nm, m) for m, nm in scenes._CUBES)["TallBox"])
    M[1, 3] += LIFT
    Ainv = np.linalg.inv(M[:, :3])
    loc = (p - M[:, 3]) @ Ainv.T
    on_face = (np.abs(np.abs(loc).max(1) - 1.0) < 1e-3)
    step = (p + 1e-3 * n - M[:, 3]) @ Ainv.T
    return int((on_face & (np.abs(step).max(1) < 1.0)).sum()), nv.shape[0]


@pytest.mark.parametrize("K", [16, 512])
def test_cornell_glass_box(pkg, oracle, scenes, gpu, plog, K):
    import torch
    kw = dict(dielectric=GLASS, dielectric_lift=LIFT, dielectric_alpha=0.1, dielectric_ior=(ETA, 1.0))
    desc = scenes.cornell_box(160, 90, **kw)
    tb = list(scenes._BSDFS).index("TallBox")
    assert desc["learned_models_nd"][tb] is not None and desc["bsdf_params"][8 * tb] == 4.0
    sc = pkg.Scene(desc)
    bare = pkg.Scene(scenes.cornell_box(160, 90, dielectric_learned=None, **kw))
    tree = _tree(pkg, sc)
    node_mix = _train(pkg, sc, tree, 6, 8, K=K)
    B = len(desc["reflectance"]) // 3
    w, m, cov, dif = scenes.diffuse_learned_bsdf(B)
    table = pkg.BsdfTable(w, m, cov, device=gpu, diffuse=dif)
    img, verts, st = sc.render(tree, node_mix, spp=4, guided=True, seed=77, learned_bsdf=table)
    assert np.isfinite(img.cpu().numpy()).all() and st["guided_queries"] > 0
    _check_producer(pkg, oracle, tree, verts, 8, 0xABF, plog, "dielectric_product")
    n_in, n_paths = _inside_inward(scenes, sc, verts)
    print(f"glass box K {K}: {n_in} saved vertices inside the box with the inward normal over {n_paths} paths")
    assert n_in >= n_paths / 100
    spp = 64
    u = _lum(sc.render(tree, None, spp=spp, guided=False, seed=4323)[0])
    for what, scene, extra, seed in (("guided", sc, {}, 2346), ("product", sc, {"learned_bsdf": table}, 2347),
                                     ("nomodel_product", bare, {"learned_bsdf": table}, 2348)):
        g = _lum(scene.render(tree, node_mix, spp=spp, guided=True, seed=seed, **extra)[0])
        assert np.isfinite(g).all()
        s = plog(f"li_dielectric_{what}_K{K}_vs_unguided_mean_sigma", _sigma(g, u), 4.0, guided=float(g.mean()),
                 unguided=float(u.mean()))
        assert s < 4.0, (what, g.mean(), u.mean())
    # transmission shows: the same scene with transmittance 0 renders another image
    opaque = pkg.Scene(scenes.cornell_box(160, 90, dielectric_transmittance=(0.0, 0.0, 0.0), **kw))
    a = sc.render(tree, None, spp=4, guided=False, seed=5)[0].clone()
    b = opaque.render(tree, None, spp=4, guided=False, seed=5)[0].clone()
    assert not torch.equal(a, b)
    # the model is used: the same render without it draws other samples
    with_model = sc.render(tree, node_mix, spp=4, guided=True, seed=78, learned_bsdf=table)[0].clone()
    img_b = bare.render(tree, node_mix, spp=4, guided=True, seed=78, learned_bsdf=table)[0].clone()
    assert not torch.equal(with_model, img_b)
    # without a model a dielectric hit takes the plain conditional and never
    # reads the caller's rows of the dielectric BSDF (a table differing only
    # there gives the same image bitwise)
    cov2 = cov.copy()
    cov2[tb] *= 0.25
    table2 = pkg.BsdfTable(w, m, cov2, device=gpu, diffuse=dif)
    img_b2 = bare.render(tree, node_mix, spp=4, guided=True, seed=78, learned_bsdf=table2)[0]
    assert torch.equal(img_b, img_b2)
