"""GPU: the Phong BSDF in the device Li (bsdf kind 3, csrc/bsdf_phong.h) and
its learned SDMM5 in the product bounce (Phong::getDMM, phong.cpp:75-90:
conditioned per bounce on (theta_i, specWeight, log exponent), pruned to 2
with the diffuse component forced, then rotate_to_wo as for the conductor).

The path-by-path comparison with the CPU Li is tests/test_gpu_li_oracle_phong.py
(unguided bit-exact, guided and product >= 99 % of the paths); here the render
is pinned by unbiasedness: a Phong
BSDF with no specular part is the diffuse BSDF, and the product render agrees
with BSDF-only sampling of the same scene (4 sigma over the pixel means, the
form of tests/test_gpu_li.py); the training records still equal the
host-routed oracle bitwise.  The BSDF itself and the conditional are pinned on
the host (tests/test_learned_nd.py) and device == host (test_gpu_learned_nd.py)."""
import numpy as np
import pytest

from test_gpu_li import _check_producer, _train, _tree

pytestmark = pytest.mark.gpu

PHONG = ("TallBox", "Floor")


def _lum(im):
    return im.cpu().numpy().mean(0).reshape(-1)


def _sigma(a, b):
    se = np.sqrt(a.var() / a.size + b.var() / b.size)
    return float(abs(a.mean() - b.mean()) / se)


def test_phong_without_specular_is_diffuse(pkg, scenes, gpu, plog):
    """ks = 0: sample / eval / pdf reduce to the diffuse BSDF's, so the
    BSDF-only image means agree (two seeds, 4 sigma)."""
    desc = scenes.cornell_box(160, 90, phong=PHONG, phong_specular=(0.0, 0.0, 0.0))
    np.testing.assert_array_equal(desc["reflectance"], scenes.cornell_box(160, 90)["reflectance"])
    ph, df = pkg.Scene(desc), pkg.Scene(scenes.cornell_box(160, 90))
    tree = _tree(pkg, ph)
    a = _lum(ph.render(tree, None, spp=64, guided=False, seed=811)[0])
    b = _lum(df.render(tree, None, spp=64, guided=False, seed=812)[0])
    assert np.isfinite(a).all()
    s = plog("li_phong_ks0_vs_diffuse_mean_sigma", _sigma(a, b), 4.0, phong=float(a.mean()), diffuse=float(b.mean()))
    assert s < 4.0, (a.mean(), b.mean())


@pytest.mark.parametrize("K", [16, 512])
def test_phong_product_render_unbiased(pkg, oracle, scenes, gpu, plog, K):
    import torch
    desc = scenes.cornell_box(160, 90, phong=PHONG)
    assert desc["learned_models_nd"][list(scenes._BSDFS).index("Floor")] is not None
    sc = pkg.Scene(desc)
    tree = _tree(pkg, sc)
    node_mix = _train(pkg, sc, tree, 6, 8, K=K)
    B = len(desc["reflectance"]) // 3
    w, m, cov, dif = scenes.diffuse_learned_bsdf(B)
    table = pkg.BsdfTable(w, m, cov, device=gpu, diffuse=dif)
    img, verts, st = sc.render(tree, node_mix, spp=4, guided=True, seed=77, learned_bsdf=table)
    assert np.isfinite(img.cpu().numpy()).all() and st["guided_queries"] > 0
    _check_producer(pkg, oracle, tree, verts, 8, 0xABF, plog, "phong_product")
    spp = 64
    g = _lum(sc.render(tree, node_mix, spp=spp, guided=True, seed=2347, learned_bsdf=table)[0])
    u = _lum(sc.render(tree, None, spp=spp, guided=False, seed=4323)[0])
    s = plog(f"li_phong_product_K{K}_vs_unguided_mean_sigma", _sigma(g, u), 4.0, product=float(g.mean()),
             unguided=float(u.mean()))
    assert s < 4.0, (g.mean(), u.mean())
    # the model is used: the same render without it (the plain conditional on
    # Phong hits) draws other samples
    bare = pkg.Scene(scenes.cornell_box(160, 90, phong=PHONG, phong_learned=None))
    with_model = sc.render(tree, node_mix, spp=4, guided=True, seed=78, learned_bsdf=table)[0].clone()
    img_b = bare.render(tree, node_mix, spp=4, guided=True, seed=78, learned_bsdf=table)[0].clone()
    assert not torch.equal(with_model, img_b)
    # without a model a Phong hit takes the plain conditional: the render is
    # finite, unbiased, and never reads the caller's rows of the Phong BSDFs
    # (a table differing only there gives the same image bitwise)
    assert np.isfinite(img_b.cpu().numpy()).all()
    cov2 = cov.copy()
    for nm in PHONG:
        cov2[list(scenes._BSDFS).index(nm)] *= 0.25
    table2 = pkg.BsdfTable(w, m, cov2, device=gpu, diffuse=dif)
    img_b2 = bare.render(tree, node_mix, spp=4, guided=True, seed=78, learned_bsdf=table2)[0]
    assert torch.equal(img_b, img_b2)
    gb = _lum(bare.render(tree, node_mix, spp=spp, guided=True, seed=2348, learned_bsdf=table)[0])
    s = plog(f"li_phong_nomodel_product_K{K}_vs_unguided_mean_sigma", _sigma(gb, u), 4.0, product=float(gb.mean()),
             unguided=float(u.mean()))
    assert s < 4.0, (gb.mean(), u.mean())
