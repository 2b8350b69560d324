"""GPU: the rough dielectric bounce of the device Li (bsdf kind 4:
li_query_kernel's roughdielectric_sample on either side, li_compact_kernel's
learned_conditional<3> without a forced lobe, li_shade_kernel's whole-sphere
eval, the crossed index, the inward normal and the path's relative index in
Russian roulette; csrc/render.hip) against the CPU restatement
(oracle/sdmm_oracle_li.inc, pinned on its own in
tests/test_li_oracle_dielectric.py), path by path, in the forms of
tests/test_gpu_li_oracle.py: unguided bit-exact, guided and product >= 99 % of
the paths within 1e-3 relative and the image mean within 0.5 %
(_compare_guided, unchanged).  Roulette is turned on (rr_depth = 2) for the
glass box and, for the first time in any path comparison, for the diffuse and
the Phong scene.

Kind 4 computes in double between float inputs and outputs; a last-bit
difference between the device's exp / log / sincos and the C library's
survives the single rounding to float with a probability of the order of
2^-29 per value, so zero mismatching paths is asserted here as in
test_gpu_roughdielectric.py::test_batch_kernel_equals_host_bitwise.

Every test counts, from the oracle's hit_bsdf / inside / comps outputs, that
the scene met the code it is about."""
import numpy as np
import pytest

from test_bsdf_roughdielectric import ETA
from test_gpu_li import _train, _tree
from test_gpu_li_oracle import SEED, SPP, _compare_guided, _device, _oracle_mixes
from test_gpu_li_oracle_phong import _second_lobe

pytestmark = pytest.mark.gpu

GLASS = ("TallBox",)


def _ids(scenes, names):
    return [list(scenes._BSDFS).index(n) for n in names]


def _glass_box(scenes, w=128, h=72, **kw):
    kw.setdefault("dielectric", GLASS)
    return scenes.cornell_box(w, h, dielectric_lift=0.02, dielectric_ior=(ETA, 1.0), **kw)


class _WithRR:
    """A scene whose render() runs with the given rr_depth: what _device is handed for the roulette cases."""

    def __init__(self, sc, rr_depth):
        self.sc, self.rr_depth = sc, rr_depth

    def render(self, *a, **kw):
        return self.sc.render(*a, rr_depth=self.rr_depth, **kw)


def _unguided(pkg, oracle, desc, rr_depth=10):
    sc = pkg.Scene(desc)
    tree = _tree(pkg, sc)
    img, rec, nv, _ = _device(_WithRR(sc, rr_depth), tree, None, False)
    aabb, child, _ = tree.nodes()
    r = oracle.li_render(desc, aabb, child, spp=SPP, seed=SEED, rr_depth=rr_depth, threads=16)
    return img, rec, nv, r, (aabb, child)


def _assert_bitwise(plog, tag, img, rec, nv, r, **counts):
    """test_phong_li_unguided_bitwise's assertions: vertex counts, live records, image."""
    sel = np.arange(rec.shape[1])[:, None] < np.minimum(nv, r["nv"])[None, :]
    bad = (nv != r["nv"]) | (np.where(sel[None], rec != r["rec"], False).any(axis=(0, 1)))
    plog(f"{tag}_mismatching_paths", int(bad.sum()), 0, paths=int(nv.shape[0]), **counts)
    print(f"{tag}: {int(bad.sum())} mismatching paths of {nv.shape[0]}; {counts}")
    np.testing.assert_array_equal(nv, r["nv"])
    plog(f"{tag}_rec_max_abs_diff", float(np.abs(rec - r["rec"])[:, sel].max()), 0.0)
    np.testing.assert_array_equal(rec[:, sel], r["rec"][:, sel])
    plog(f"{tag}_image_max_abs_diff", float(np.abs(img - r["image"]).max()), 0.0)
    np.testing.assert_array_equal(img, r["image"])


def _glass_counts(r, ids):
    """From the oracle's outputs: paths with a hit from inside; saved vertices
    with the flipped normal; reflected and transmitted dielectric bounces.  No
    delta lobe in these scenes, so saved vertex v is bounce v; the saved normal
    is the one on wi's side, so a saved direction below it was transmitted."""
    V = r["rec"].shape[1]
    live = np.arange(V)[:, None] < r["nv"][None, :]
    glass = np.isin(r["hit_bsdf"][:V], ids) & live
    inside = (r["inside"][:V] == 1) & live
    below = (r["rec"][10:13] * r["rec"][13:16]).sum(0) < 0
    return {"inside_paths": int(inside.any(0).sum()), "flipped_normal_vertices": int(inside.sum()),
            "saved_vertices": int(live.sum()), "reflected": int((glass & ~below).sum()),
            "transmitted": int((glass & below).sum())}


def _roulette_deaths(r, r10):
    """Paths the roulette ended: fewer live bounces than the rr_depth = 10 run
    of the same seed (the uniforms are counter-based, so until its death a path
    is that run's path)."""
    n, n10 = (r["hit_bsdf"] >= 0).sum(0), (r10["hit_bsdf"] >= 0).sum(0)
    assert (n <= n10).all()
    return int((n < n10).sum())


@pytest.mark.parametrize("alpha", [0.1, 0.3])
def test_glass_box_li_unguided_bitwise(pkg, oracle, scenes, gpu, plog, alpha):
    """A rough-dielectric tall box: the device Li equals the CPU Li bit for
    bit, unguided -- vertex counts, live records (the inward normal inside the
    glass among them), image."""
    desc = _glass_box(scenes, dielectric_alpha=alpha)
    img, rec, nv, r, _ = _unguided(pkg, oracle, desc)
    c = _glass_counts(r, _ids(scenes, GLASS))
    P = nv.shape[0]
    assert c["inside_paths"] >= P // 100 and c["flipped_normal_vertices"] >= c["saved_vertices"] // 100, c
    assert c["reflected"] > 0 and c["transmitted"] > 0, c
    _assert_bitwise(plog, f"li_dielectric_a{alpha}_unguided", img, rec, nv, r, **c)


def test_glass_box_li_roulette_bitwise(pkg, oracle, scenes, gpu, plog):
    """The same with rr_depth = 2: q = min(max(thr) * eta^2, 0.95) with the
    path's relative index (sdmm_proc.cpp:788, :864).  The scene pins the
    factor: with eta taken as 1 the oracle itself ends other paths."""
    desc = _glass_box(scenes, dielectric_alpha=0.1)
    img, rec, nv, r, (aabb, child) = _unguided(pkg, oracle, desc, rr_depth=2)
    r10 = oracle.li_render(desc, aabb, child, spp=SPP, seed=SEED, threads=16)
    r1 = oracle.li_render(desc, aabb, child, spp=SPP, seed=SEED, rr_depth=2, threads=16, rr_eta_one=True)
    c = _glass_counts(r, _ids(scenes, GLASS))
    c["roulette_deaths"] = _roulette_deaths(r, r10)
    c["paths_changed_by_eta"] = int((r1["nv"] != r["nv"]).sum())
    P = nv.shape[0]
    assert c["roulette_deaths"] >= P // 20 and c["paths_changed_by_eta"] >= 1 and c["inside_paths"] >= P // 100, c
    _assert_bitwise(plog, "li_dielectric_rr2_unguided", img, rec, nv, r, **c)


@pytest.mark.parametrize("what", ["diffuse", "phong"])
def test_roulette_li_unguided_bitwise(pkg, oracle, scenes, gpu, plog, what):
    """rr_depth = 2 on the plain Cornell box and on the Phong scene of
    test_gpu_li_oracle_phong.py: the roulette's uniform (dimension 6), the
    0.95 cap and thr /= q, bit for bit."""
    desc = scenes.cornell_box(128, 72, phong=() if what == "diffuse" else ("TallBox", "Floor"))
    img, rec, nv, r, (aabb, child) = _unguided(pkg, oracle, desc, rr_depth=2)
    r10 = oracle.li_render(desc, aabb, child, spp=SPP, seed=SEED, threads=16)
    deaths = _roulette_deaths(r, r10)
    # survivors were rescaled: some saved throughput differs from the run without roulette
    V = rec.shape[1]
    both = np.arange(V)[:, None] < np.minimum(r["nv"], r10["nv"])[None, :]
    rescaled = int((np.where(both[None], r["rec"][3:6] != r10["rec"][3:6], False).any(axis=(0, 1))).sum())
    assert deaths >= nv.shape[0] // 20 and rescaled > 0, (deaths, rescaled)
    _assert_bitwise(plog, f"li_{what}_rr2_unguided", img, rec, nv, r, roulette_deaths=deaths, rescaled_paths=rescaled)


@pytest.mark.parametrize("zero", ["transmittance", "reflectance"])
def test_glass_box_zero_lobe_unguided_bitwise(pkg, oracle, scenes, gpu, plog, zero):
    """specularTransmittance 0, then specularReflectance 0: the liveness rule
    (alive while either is non-zero) and samples of the black lobe, which end
    the path with weight 0."""
    key = "dielectric_transmittance" if zero == "transmittance" else "dielectric_specular"
    desc = _glass_box(scenes, dielectric_alpha=0.1, **{key: (0.0, 0.0, 0.0)})
    tb = _ids(scenes, GLASS)[0]
    trans, spec = desc["reflectance"].reshape(-1, 3)[tb], desc["bsdf_params"].reshape(-1, 8)[tb, 1:4]
    assert ((trans if zero == "transmittance" else spec) == 0).all() and (trans + spec == 1).all()
    img, rec, nv, r, _ = _unguided(pkg, oracle, desc)
    c = _glass_counts(r, [tb])
    # loop heads that were live on the glass and saved no vertex (vertex v is bounce v): the black
    # lobe was drawn, or the sample was void
    V = rec.shape[1]
    glass_live = r["hit_bsdf"][:V] == tb
    c["glass_bounces"] = int(glass_live.sum())
    c["zero_weight_ends"] = int((glass_live & ~(np.arange(V)[:, None] < r["nv"][None, :])).sum())
    assert c["glass_bounces"] > nv.shape[0] // 20 and c["zero_weight_ends"] > c["glass_bounces"] // 100, c
    if zero == "transmittance":
        assert c["transmitted"] == 0 and c["inside_paths"] == 0 and c["reflected"] > 0, c
    else:
        assert c["reflected"] == 0 and c["transmitted"] > 0 and c["inside_paths"] > 0, c
    _assert_bitwise(plog, f"li_dielectric_zero_{zero}_unguided", img, rec, nv, r, **c)


def _guided(pkg, oracle, scenes, gpu, desc, K, product):
    sc = pkg.Scene(desc)
    tree = _tree(pkg, sc)
    node_mix = _train(pkg, sc, tree, 4, 8, K=K)
    assert any(m is not None and m.K == K for m in node_mix)
    learned = table = None
    if product:
        learned = scenes.diffuse_learned_bsdf(len(desc["reflectance"]) // 3)
        table = pkg.BsdfTable(*learned[:3], device=gpu, diffuse=learned[3])
    img, rec, nv, _ = _device(sc, tree, node_mix, True, table=table)
    aabb, child, _ = tree.nodes()
    r = oracle.li_render(desc, aabb, child, node_mix=_oracle_mixes(oracle, node_mix), guided=True, spp=SPP,
                         seed=SEED, learned=learned, threads=16)
    return img, rec, nv, r


def _guide_counts(r, ids):
    """Guide samples (comps >= 0) taken on hits of the BSDFs ids: from outside,
    from inside, and those whose direction went below the surface it met (a
    transmitted eval)."""
    V = r["rec"].shape[1]
    live = np.arange(V)[:, None] < r["nv"][None, :]
    g = (r["comps"][:V] >= 0) & np.isin(r["hit_bsdf"][:V], ids)
    below = (r["rec"][10:13] * r["rec"][13:16]).sum(0) < 0
    side = r["inside"][:V]
    return {"guide_outside": int((g & (side == 0)).sum()), "guide_inside": int((g & (side == 1)).sum()),
            "guide_transmitted": int((g & live & below).sum())}


def test_glass_box_guided_li_matches_oracle(pkg, oracle, scenes, gpu, plog):
    """Plain guiding over the glass box: the shade kernel's whole-sphere
    roughdielectric_eval_pdf and roughdielectric_crossed_eta at the guide's
    direction.

    alpha 0.3, not 0.1: a guide direction that differs by 1e-5 between device
    and oracle moves the Beckmann density by about 2 theta_m / alpha^2 x 1e-5
    relative; at theta_m = 3 alpha that is 6e-5 / alpha -- 2e-4 at 0.3, inside
    _compare_guided's 1e-3 with room for the half-vector Jacobian, and 6e-4 at
    0.1, which is not."""
    desc = _glass_box(scenes, dielectric_alpha=0.3)
    img, rec, nv, r = _guided(pkg, oracle, scenes, gpu, desc, 16, product=False)
    c = _guide_counts(r, _ids(scenes, GLASS))
    print("glass box guided:", c)
    assert c["guide_outside"] > 0 and c["guide_inside"] > 0 and c["guide_transmitted"] > 0, c
    plog("li_dielectric_guided_transmitted_guide_samples", c["guide_transmitted"], 1, lower=True, **c)
    _compare_guided(oracle, plog, "li_dielectric_guided", img, rec, nv, r)


def _second_lobe_outside(r, ids):
    """_second_lobe at hits from outside: from inside a dielectric has no
    learned BSDF, and the plain conditional's index k may be odd as well."""
    return _second_lobe({**r, "hit_bsdf": np.where(r["inside"] == 1, -1, r["hit_bsdf"])}, ids)


def _inside_plain_conditional(r, ids):
    """Guide samples on hits of ids from inside in a product render: the plain
    conditional's component indices (k < K; the product's are k * 2 + j, so
    this counts the bounces, not their index)."""
    V = r["rec"].shape[1]
    return int(((r["comps"][:V] >= 0) & np.isin(r["hit_bsdf"][:V], ids) & (r["inside"][:V] == 1)).sum())


@pytest.mark.parametrize("K,w,h", [(16, 128, 72), (512, 64, 36)])
def test_glass_box_product_li_matches_oracle(pkg, oracle, scenes, gpu, plog, K, w, h):
    """sampleProduct over the glass box with the shipped SDMM5: a hit from
    outside conditions it on (theta_i, alpha, eta), prunes to 2 without a
    forced lobe and rotates to wi (RoughDielectric::getDMM,
    roughdielectric.cpp:198-211); a hit from inside has no learned BSDF (:199)
    and takes the plain conditional with h 0.5.  alpha 0.3: see
    test_glass_box_guided_li_matches_oracle."""
    desc = _glass_box(scenes, w, h, dielectric_alpha=0.3)
    tb = _ids(scenes, GLASS)
    assert desc["learned_models_nd"][tb[0]] is not None
    img, rec, nv, r = _guided(pkg, oracle, scenes, gpu, desc, K, product=True)
    n2, nin = _second_lobe_outside(r, tb), _inside_plain_conditional(r, tb)
    plog(f"li_dielectric_product_K{K}_second_lobe_samples", n2, 1, lower=True)
    plog(f"li_dielectric_product_K{K}_inside_plain_conditional_samples", nin, 1, lower=True)
    print(f"glass box product K {K}: second-lobe samples {n2}, guide samples from inside {nin}")
    assert n2 > 0 and nin > 0
    # a weak guard beside _compare_guided: the plain conditional's index stays below K, a product's index
    # k * 2 + j may or may not -- none of K or more occurred from inside
    inside_glass = (r["inside"] == 1) & np.isin(r["hit_bsdf"], tb)
    assert r["comps"][inside_glass].max() < K
    _compare_guided(oracle, plog, f"li_dielectric_product_K{K}", img, rec, nv, r)


def test_glass_box_without_learned_model_plain_conditional(pkg, oracle, scenes, gpu, plog):
    """A rough dielectric with no learned model (m_sdmm == nullptr,
    roughdielectric.cpp:199): its product bounces take the plain conditional
    with h 0.5, the query rows still max(M, 2) lobes wide."""
    desc = _glass_box(scenes, dielectric_alpha=0.3, dielectric_learned=None)
    assert "learned_models_nd" not in desc
    img, rec, nv, r = _guided(pkg, oracle, scenes, gpu, desc, 16, product=True)
    tb = _ids(scenes, GLASS)
    on_glass = np.isin(r["hit_bsdf"], tb)
    n = int(((r["comps"] >= 0) & on_glass).sum())
    assert n > 0 and r["comps"][on_glass].max() < 16
    plog("li_dielectric_no_model_guide_samples_on_glass", n, 1, lower=True)
    _compare_guided(oracle, plog, "li_dielectric_no_model", img, rec, nv, r)


def test_mixed_conductor_phong_dielectric_product(pkg, oracle, scenes, gpu, plog):
    """A conductor floor, a Phong short box and a glass tall box in one
    scene, all with the product: the SDMM4 table, the two SDMM5 models of one
    table and the shared query rows work together."""
    desc = _glass_box(scenes, conductor=("Floor",), phong=("ShortBox",), dielectric_alpha=0.3)
    fl, sb, tb = _ids(scenes, ("Floor", "ShortBox", "TallBox"))
    assert desc["learned_models"][fl] is not None
    assert desc["learned_models_nd"][sb] is not None and desc["learned_models_nd"][tb] is not None
    assert desc["learned_models_nd"][sb][1].shape == desc["learned_models_nd"][tb][1].shape
    assert not np.array_equal(desc["learned_models_nd"][sb][1], desc["learned_models_nd"][tb][1])
    img, rec, nv, r = _guided(pkg, oracle, scenes, gpu, desc, 16, product=True)
    n = {"conductor": _second_lobe(r, [fl]), "phong": _second_lobe(r, [sb]),
         "dielectric": _second_lobe_outside(r, [tb])}
    for k, v in n.items():
        plog(f"li_mixed3_{k}_second_lobe_samples", v, 1, lower=True)
    print("mixed scene second-lobe samples:", n)
    assert min(n.values()) > 0, n
    _compare_guided(oracle, plog, "li_mixed_conductor_phong_dielectric_product", img, rec, nv, r)
