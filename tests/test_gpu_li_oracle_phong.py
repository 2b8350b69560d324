"""GPU: the Phong bounce of the device Li (bsdf kind 3: li_query_kernel's
phong_sample, li_compact_kernel's learned_conditional<3> with the diffuse lobe
forced, li_shade_kernel's phong_eval_pdf; csrc/render.hip) against the CPU
restatement (oracle/sdmm_oracle_li.inc: li_phong_*, li_learned_nd_conditional,
pinned on their own in tests/test_li_oracle_phong.py), path by path, in the
forms of tests/test_gpu_li_oracle.py: unguided bit-exact, guided and product
>= 99 % of the paths within 1e-3 relative and the image mean within 0.5 %
(_compare_guided, unchanged).

What a path comparison sees that an unbiasedness check cannot: the local
frame the kernels hand to the BSDF, the rho row and the bp offsets, the
sample's weight and pdf carried from the loop head to the shade kernel, the
liveness rule of kind 3, and in the product bounce the condition vector, the
model table's offset and stride and the query's row of the extended table."""
import numpy as np
import pytest

from test_gpu_li import _train, _tree
from test_gpu_li_oracle import SEED, SPP, _compare_guided, _device, _oracle_mixes

pytestmark = pytest.mark.gpu

PHONG = ("TallBox", "Floor")


def _ids(scenes, names):
    return [list(scenes._BSDFS).index(n) for n in names]


def _black_base(scenes, desc):
    """The Phong BSDFs of desc with their diffuse reflectance zeroed: the
    specular sampling weight sAvg / (0 + sAvg) is exactly 1."""
    bp = desc["bsdf_params"].reshape(-1, 8).copy()
    refl = desc["reflectance"].reshape(-1, 3).copy()
    for b in _ids(scenes, PHONG):
        bp[b], refl[b] = scenes.phong_params((0.0, 0.0, 0.0), tuple(bp[b, 1:4]), float(bp[b, 4]))
        assert bp[b, 5] == 1.0 and (refl[b] == 0.0).all()
    desc["bsdf_params"] = bp.reshape(-1)
    desc["reflectance"] = refl.reshape(-1)
    return desc


@pytest.mark.parametrize("specular,exponent,black", [(0.4, 30.0, False), (0.7, 1000.0, False), (0.4, 30.0, True)],
                         ids=["ks0.4_n30", "ks0.7_n1000", "black_base"])
def test_phong_li_unguided_bitwise(pkg, oracle, scenes, gpu, plog, specular, exponent, black):
    """Phong BSDFs on the tall box and the floor: the device Li equals the CPU
    Li bit for bit, unguided -- vertex counts, live records, image.  Both
    sides round a double pow / sincos to float (the conductor test's premise);
    black_base: a zero diffuse reflectance, so only the specular lobe is ever
    sampled and the part of it below the horizon ends the path."""
    desc = scenes.cornell_box(128, 72, phong=PHONG, phong_specular=(specular,) * 3, phong_exponent=exponent)
    if black:
        desc = _black_base(scenes, desc)
    tag = f"li_phong_ks{specular}_n{int(exponent)}{'_black' if black else ''}_unguided"
    sc = pkg.Scene(desc)
    tree = _tree(pkg, sc)
    img, rec, nv, _ = _device(sc, tree, None, False)
    aabb, child, _ = tree.nodes()
    r = oracle.li_render(desc, aabb, child, spp=SPP, seed=SEED, threads=8)
    # the Phong quads are hit and scatter on
    ph = np.isin(r["hit_bsdf"], _ids(scenes, PHONG))
    assert ph[0].mean() > 0.05 and ph[1:].sum() > nv.shape[0] // 4
    sel = np.arange(rec.shape[1])[:, None] < np.minimum(nv, r["nv"])[None, :]
    bad = (nv != r["nv"]) | (np.where(sel[None], rec != r["rec"], False).any(axis=(0, 1)))
    plog(f"{tag}_mismatching_paths", int(bad.sum()), 0, paths=int(nv.shape[0]), phong_bounces=int(ph.sum()))
    np.testing.assert_array_equal(nv, r["nv"])
    plog(f"{tag}_rec_max_abs_diff", float(np.abs(rec - r["rec"])[:, sel].max()), 0.0)
    np.testing.assert_array_equal(rec[:, sel], r["rec"][:, sel])
    plog(f"{tag}_image_max_abs_diff", float(np.abs(img - r["image"]).max()), 0.0)
    np.testing.assert_array_equal(img, r["image"])


def test_phong_guided_li_matches_oracle(pkg, oracle, scenes, gpu, plog):
    """Plain guiding (no product) over Phong BSDFs: the shade kernel's
    phong_eval_pdf at the guide's direction and the MIS mix."""
    desc = scenes.cornell_box(128, 72, phong=PHONG)
    sc = pkg.Scene(desc)
    tree = _tree(pkg, sc)
    node_mix = _train(pkg, sc, tree, 4, 8, K=16)
    img, rec, nv, _ = _device(sc, tree, node_mix, True)
    aabb, child, _ = tree.nodes()
    r = oracle.li_render(desc, aabb, child, node_mix=_oracle_mixes(oracle, node_mix), guided=True, spp=SPP,
                         seed=SEED, threads=16)
    _compare_guided(oracle, plog, "li_phong_guided", img, rec, nv, r)
    ph = np.isin(r["hit_bsdf"], _ids(scenes, PHONG))
    assert ((r["comps"] >= 0) & ph).sum() > 0           # guide samples taken on Phong hits


def _product(pkg, oracle, scenes, gpu, desc, K):
    sc = pkg.Scene(desc)
    tree = _tree(pkg, sc)
    node_mix = _train(pkg, sc, tree, 4, 8, K=K)
    assert any(m is not None and m.K == K for m in node_mix)
    learned = scenes.diffuse_learned_bsdf(len(desc["reflectance"]) // 3)
    table = pkg.BsdfTable(*learned[:3], device=gpu, diffuse=learned[3])
    img, rec, nv, _ = _device(sc, tree, node_mix, True, table=table)
    aabb, child, _ = tree.nodes()
    r = oracle.li_render(desc, aabb, child, node_mix=_oracle_mixes(oracle, node_mix), guided=True, spp=SPP,
                         seed=SEED, learned=learned, threads=16)
    return img, rec, nv, r


def _second_lobe(r, ids):
    """Guided samples from the second lobe of a conditioned model at hits of
    the BSDFs `ids`: with max(M, 2) = 2 lobes per row the odd component
    indices (the diffuse rows hold one lobe: theirs are even)."""
    comps = r["comps"]
    return int(((comps >= 0) & (comps % 2 != 0) & np.isin(r["hit_bsdf"], ids)).sum())


@pytest.mark.parametrize("K,w,h", [(16, 128, 72), (512, 64, 36)])
def test_phong_product_li_matches_oracle(pkg, oracle, scenes, gpu, plog, K, w, h):
    """sampleProduct over Phong BSDFs with the shipped SDMM5: each Phong
    bounce conditions it on (theta_i, max specular channel, log max(1,
    exponent)), prunes to 2 with the diffuse component forced, rotates to wi
    (Phong::getDMM, phong.cpp:75-90; sdmm_proc.cpp:340-355).  Exponent 30: a
    guided direction 1e-5 apart between device and oracle moves alpha^n by
    about n x 1e-5 = 3e-4 relative, inside _compare_guided's 1e-3."""
    desc = scenes.cornell_box(w, h, phong=PHONG)
    assert desc["learned_models_nd"][_ids(scenes, ("Floor",))[0]] is not None
    assert desc["bsdf_params"].reshape(-1, 8)[_ids(scenes, ("Floor",))[0], 4] == 30.0
    img, rec, nv, r = _product(pkg, oracle, scenes, gpu, desc, K)
    _compare_guided(oracle, plog, f"li_phong_product_K{K}", img, rec, nv, r)
    n2 = _second_lobe(r, _ids(scenes, PHONG))
    plog(f"li_phong_product_K{K}_second_lobe_samples", n2, 1, lower=True)
    assert n2 > 0


def test_phong_without_learned_model_plain_conditional(pkg, oracle, scenes, gpu, plog):
    """A Phong BSDF with no learned model (m_sdmm == nullptr: getDMM returns
    false, phong.cpp:78-80): its product bounces fall back to the plain
    conditional with h 0.5 (sdmm_proc.cpp:383) -- device == CPU Li, the query
    rows still max(M, 2) lobes wide."""
    desc = scenes.cornell_box(128, 72, phong=PHONG, phong_learned=None)
    assert "learned_models_nd" not in desc
    img, rec, nv, r = _product(pkg, oracle, scenes, gpu, desc, 16)
    _compare_guided(oracle, plog, "li_phong_no_model", img, rec, nv, r)
    ph = np.isin(r["hit_bsdf"], _ids(scenes, PHONG))
    assert ((r["comps"] >= 0) & ph).sum() > 0


def test_mixed_conductor_and_phong_product(pkg, oracle, scenes, gpu, plog):
    """A rough conductor (the tall box) and a Phong BSDF (the floor) in one
    scene: both model tables are live and their per-bounce lobes share the
    query rows of the extended table.  Both materials' bounces draw product
    samples from their conditioned models."""
    desc = scenes.cornell_box(128, 72, conductor=("TallBox",), phong=("Floor",))
    tb, fl = _ids(scenes, ("TallBox", "Floor"))
    assert desc["learned_models"][tb] is not None and desc["learned_models"][fl] is None
    assert desc["learned_models_nd"][fl] is not None and desc["learned_models_nd"][tb] is None
    img, rec, nv, r = _product(pkg, oracle, scenes, gpu, desc, 16)
    _compare_guided(oracle, plog, "li_mixed_conductor_phong_product", img, rec, nv, r)
    nc, npg = _second_lobe(r, [tb]), _second_lobe(r, [fl])
    plog("li_mixed_conductor_second_lobe_samples", nc, 1, lower=True)
    plog("li_mixed_phong_second_lobe_samples", npg, 1, lower=True)
    assert nc > 0 and npg > 0
