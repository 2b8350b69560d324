"""CPU: the oracle's Phong BSDF and N-D learned conditional (oracle/
sdmm_oracle_li.inc: li_phong_eval_pdf / li_phong_sample, li_learned_nd_
conditional) -- the restatements the device Li is compared with in
tests/test_gpu_li_oracle_phong.py -- shown right on their own:

  * bit for bit equal to the library's host code (csrc/bsdf_phong.h,
    csrc/learned_bsdf.h through sdmm_bsdf_phong_host / sdmm_learned_conditional;
    both run here with the same C library, so a difference is one of code);
  * against phong.cpp:171-289 in float64 (test_learned_nd.py's restatement and
    tolerances);
  * the oracle's Li on a Phong face against the directional albedo by
    quadrature -- a check that does not go through the library at all."""
import numpy as np
import pytest

from test_learned_bsdf import _wi
from test_learned_nd import _four, _phong_eval_pdf64, _phong_sample64
from test_li_oracle import _furnace

ONE_M = np.float32(1.0 - 2.0 ** -24)      # the largest uniform below 1


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    """(wo, value, pdf) triples equal bit for bit (NaN and the sign of zero included)."""
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _mat(scenes, diffuse, specular, exponent):
    bp, rho = scenes.phong_params((diffuse,) * 3 if np.isscalar(diffuse) else diffuse,
                                  (specular,) * 3 if np.isscalar(specular) else specular, exponent)
    return bp, rho


def test_oracle_phong_equals_host_bitwise(pkg, oracle, scenes):
    """sample (wo, weight, pdf) and eval / pdf at a given wo: or_bsdf_phong ==
    sdmm_bsdf_phong_host on every bit, over random inputs and the edges of the
    two-lobe sample (the lobe choice at u0 == weight, weight 0 and 1, exponent
    0 .. 1000, u1 at both ends, grazing and back-facing wi, a wo outside the
    specular lobe, a specular sample below the horizon)."""
    rng = np.random.default_rng(2024)
    mism = n_calls = 0

    def both(bp, rho, wi, **kw):
        nonlocal mism, n_calls
        a, b = pkg.bsdf_phong_host(bp, rho, wi, **kw), oracle.bsdf_phong(bp, rho, wi, **kw)
        n_calls += 1
        mism += not _same(a, b)
        return a, b

    # random inputs
    mats = [_mat(scenes, (0.5, 0.4, 0.3), (0.3, 0.2, 0.4), 30.0), _mat(scenes, (0.725, 0.71, 0.68), 0.4, 10.0),
            _mat(scenes, 0.2, (0.7, 0.6, 0.5), 1.0), _mat(scenes, 0.5, 0.0, 30.0), _mat(scenes, 0.0, 0.6, 5.0),
            _mat(scenes, 0.1, 0.7, 1000.0)]
    W, WO = _wi(rng, 4000), _wi(rng, 4000)
    U = rng.uniform(0, 1, (4000, 2)).astype(np.float32)
    for i in range(4000):
        bp, rho = mats[i % len(mats)]
        (wo, _, _), _ = both(bp, rho, W[i], u=U[i])
        both(bp, rho, W[i], wo=WO[i])
        both(bp, rho, W[i], wo=wo)
    # the edges, crossed
    wis = [np.float32([0.0, 0.0, 1.0]), np.float32([0.48, -0.64, 0.6]),
           np.float32([np.sqrt(1.0 - 1e-8), 0.0, 1e-4]), np.float32([0.0, -np.sqrt(1.0 - 1e-8), 1e-4]),
           np.float32([0.6, 0.0, -0.8]), np.float32([1.0, 0.0, 0.0])]
    wos = [np.float32([0.0, 0.0, 1.0]), np.float32([-0.48, 0.64, 0.6]), np.float32([0.8, 0.0, 0.6]),
           np.float32([0.0, 1.0, 0.0]), np.float32([0.0, 0.6, -0.8])]
    n_void_spec = 0
    for exponent in (0.0, 1.0, 30.0, 1000.0):
        for diffuse, specular in ((0.5, 0.3), (0.5, 0.0), (0.0, 0.6)):
            bp, rho = _mat(scenes, diffuse, specular, exponent)
            ssw = np.float32(bp[5])
            assert (ssw == 0.0) == (specular == 0.0) and (ssw == 1.0) == (diffuse == 0.0)
            u0s = {np.float32(0.0), ssw, np.nextafter(ssw, np.float32(2.0)), np.float32(0.5), ONE_M}
            for wi in wis:
                for u0 in sorted(u0s):
                    for u1 in (np.float32(0.0), np.float32(0.3), ONE_M):
                        if u0 > 1.0:
                            continue
                        (wo, val, pdf), _ = both(bp, rho, wi, u=np.float32([u0, u1]))
                        spec = u0 <= ssw and ssw > 0
                        if spec and wi[2] > 0 and wo[2] <= 0:
                            n_void_spec += 1
                            assert pdf == 0.0 and (val == 0.0).all()
                for wo in wos:
                    both(bp, rho, wi, wo=wo)
    # a wo with alpha <= 0: the diffuse term alone
    bp, rho = _mat(scenes, (0.5, 0.4, 0.3), 0.3, 30.0)
    wi = wo = np.float32([0.8, 0.0, 0.6])
    assert np.dot(wo, [-wi[0], -wi[1], wi[2]]) < 0
    (_, f, p), _ = both(bp, rho, wi, wo=wo)
    inv_pi = np.float32(0.31830988618379067154)
    np.testing.assert_array_equal(f, (rho * inv_pi) * wo[2])
    assert np.float32(p) == (np.float32(1) - bp[5]) * (inv_pi * wo[2])
    # a specular sample below the horizon (grazing wi, low exponent): void on both sides
    bp, rho = _mat(scenes, 0.2, 0.6, 1.0)
    wi = np.float32([np.sqrt(1.0 - 1e-8), 0.0, 1e-4])
    found = 0
    for u0 in np.linspace(0.0, float(bp[5]), 16, dtype=np.float32):
        for u1 in np.float32([0.05, 0.3, 0.7]):
            (wo, val, pdf), (wo2, val2, pdf2) = both(bp, rho, wi, u=np.float32([u0, u1]))
            if wo[2] <= 0:
                found += 1
                assert pdf == 0.0 and pdf2 == 0.0 and (val == 0.0).all() and (val2 == 0.0).all()
    assert found > 0 and n_void_spec > 0
    print(f"oracle Phong vs host: {mism} mismatches in {n_calls} calls, {found + n_void_spec} void specular samples")
    assert mism == 0


def test_oracle_phong_matches_float64(oracle, scenes):
    """The oracle's entry through the checks of test_learned_nd.py::
    test_phong_host_matches_float64, with that test's inputs and tolerances
    (value / pdf rtol 1e-5, wo atol 2e-6 + 3e-7 / sqrt(1 - p); derived there)."""
    rng = np.random.default_rng(17)
    mats = [scenes.phong_params((0.5, 0.4, 0.3), (0.3, 0.2, 0.4), 30.0),
            scenes.phong_params((0.725, 0.71, 0.68), (0.4, 0.4, 0.4), 10.0),
            scenes.phong_params((0.2, 0.2, 0.2), (0.7, 0.6, 0.5), 1.0),
            scenes.phong_params((0.5, 0.5, 0.5), (0.0, 0.0, 0.0), 30.0)]
    W = _wi(rng, 2000)
    U = rng.uniform(0, 1, (2000, 2)).astype(np.float32)
    n_spec = n_void = 0
    for i, (wi, u) in enumerate(zip(W, U)):
        bp, rho = mats[i % 4]
        if i % 50 == 0:
            u = np.float32([bp[5], u[1]])                 # u0 == weight: still the specular lobe
        wo, value, pdf = oracle.bsdf_phong(bp, rho, wi, u=u)
        b64, r64, wi64 = bp.astype(np.float64), rho.astype(np.float64), wi.astype(np.float64)
        wo64, spec, s = _phong_sample64(b64, wi64, u)
        assert spec == (u[0] <= bp[5] and bp[5] > 0)
        n_spec += spec
        np.testing.assert_allclose(wo, wo64, rtol=0, atol=2e-6 + 3e-7 / max(s, 1e-30))
        f, p = _phong_eval_pdf64(b64, r64, wi64, wo.astype(np.float64))
        if wo[2] <= 0:
            n_void += 1
            assert spec and pdf == 0.0 and (value == 0.0).all()
            continue
        np.testing.assert_allclose(pdf, p, rtol=1e-5)
        np.testing.assert_allclose(value, f / p, rtol=1e-5, atol=1e-30)
        for wg in (wo, _wi(rng, 1)[0]):
            _, fe, pe = oracle.bsdf_phong(bp, rho, wi, wo=wg)
            f, p = _phong_eval_pdf64(b64, r64, wi64, wg.astype(np.float64))
            np.testing.assert_allclose(pe, p, rtol=1e-5)
            np.testing.assert_allclose(fe, f, rtol=1e-5, atol=1e-30)
        _, fe, pe = oracle.bsdf_phong(bp, rho, wi, wo=np.float32([wo[0], wo[1], -wo[2]]))
        assert pe == 0.0 and (fe == 0.0).all()             # wo.z <= 0
    assert n_spec > 300 and n_void > 0


def _bad_sdd():
    """_four() with component 2's Schur complement S_dd - S_dc S_cc^-1 S_cd not
    PD (S_cc itself is): (0.06 / 0.3)^2 = 0.04 > S_dd[0, 0] = 0.02."""
    w, mu, cov, _ = _four()
    cov = cov.reshape(4, 5, 5).copy()
    cov[2, 0, 3] = cov[2, 3, 0] = 0.06
    return w, mu, cov.reshape(4, 25)


def _all_bad():
    w, mu, cov, _ = _four()
    cov = cov.reshape(4, 5, 5).copy()
    cov[:, 0, 1] = cov[:, 1, 0] = 0.07
    return w, mu, cov.reshape(4, 25)


def test_oracle_nd_conditional_equals_host_bitwise(pkg, oracle, scenes):
    """or_learned_nd_conditional == sdmm_learned_conditional on every bit: the
    shipped Phong SDMM5 (C = 3) and the conductor's SDMM4 (C = 2), every keep
    / force rule, directions at the pole, on and below the horizon, components
    with a non-PD S_cc or S'_dd (also as the forced one), all of them invalid.
    The host ABI rejects force >= M; the oracle treats such a force as no
    valid forced component, i.e. as force -1.  At C = 2, force -1 the result is
    or_learned4_conditional's as well."""
    rng = np.random.default_rng(99)
    dirs = list(_wi(rng, 40)) + [np.float32([0.0, 0.0, 1.0]), np.float32([1.0, 0.0, 0.0]),
                                 np.float32([0.6, 0.0, -0.8]), np.float32([0.0, np.sqrt(1 - 1e-8), 1e-4]),
                                 np.float32([np.sin(0.5), 0.0, np.cos(0.5)])]
    rest3 = [(0.4, float(np.log(30.0))), (0.2, 0.0), (0.7, float(np.log(1000.0))), (0.45, 2.3)]
    rest2 = [(0.03,), (0.2,), (0.6,)]
    models = {"phong": (scenes.load_learned_nd(), rest3), "conductor": (scenes.load_learned(), rest2),
              "four": (_four()[:3], rest3), "bad_scc": (_four(bad_scc=True)[:3], rest3),
              "bad_sdd": (_bad_sdd(), rest3), "all_bad": (_all_bad(), rest3)}
    mism = n_calls = 0
    counts = {}
    for name, (m, rests) in models.items():
        L = pkg.LearnedBSDFND(*m)
        M = L.M
        for keep in (0, 1, 2, 3):
            for force in (-1, 0, 1, M, M + 3):
                for wl in dirs:
                    for rest in rests:
                        b = oracle.learned_nd_conditional(m, rest, wl, keep, force)
                        if force >= M:
                            with pytest.raises(pkg.SDMMError):
                                L.conditional(rest, wl, keep, force)
                            a = L.conditional(rest, wl, keep, -1)
                        else:
                            a = L.conditional(rest, wl, keep, force)
                        n_calls += 1
                        mism += not _same(a, b)
                        counts[name, len(b[0])] = counts.get((name, len(b[0])), 0) + 1
                        if not wl[2] > 0 or name == "all_bad":
                            assert len(a[0]) == len(b[0]) == 0
                        if L.C == 2 and force == -1 and keep >= 1:
                            assert _same(b, oracle.learned4_conditional(m, rest[0], wl, keep))
    print(f"oracle N-D conditional vs host: {mism} mismatches in {n_calls} calls; lobes written {counts}")
    assert mism == 0
    # the cases meant were met: full and partial selections, and the invalid components dropped
    assert counts["phong", 2] > 0 and counts["phong", 4] > 0 and counts["conductor", 3] > 0
    wl, rest = np.float32([np.sin(0.5), 0.0, np.cos(0.5)]), (0.45, 2.3)
    assert len(oracle.learned_nd_conditional(_four()[:3], rest, wl, 0, -1)[0]) == 4
    assert len(oracle.learned_nd_conditional(_four(bad_scc=True)[:3], rest, wl, 0, -1)[0]) == 3
    assert len(oracle.learned_nd_conditional(_bad_sdd(), rest, wl, 0, -1)[0]) == 3
    # the forced component being the invalid one: plain pruning
    plain = oracle.learned_nd_conditional(_four(bad_scc=True)[:3], rest, wl, 2, -1)
    assert _same(oracle.learned_nd_conditional(_four(bad_scc=True)[:3], rest, wl, 2, 1), plain)
    # and a valid one changes the selection
    assert not _same(oracle.learned_nd_conditional(_four()[:3], rest, wl, 2, 1),
                     oracle.learned_nd_conditional(_four()[:3], rest, wl, 2, -1))


def _phong_albedo(cos_i, ks, n, rho):
    """int f(wi, wo) dwo, f = (ks (n + 2) / (2 pi) alpha^n + rho / pi) cos(theta_o),
    alpha = max(0, wo . reflect(wi)), in float64.  In polar coordinates (a, phi)
    about the mirror direction R (at angle theta_i from the normal) cos(theta_o) =
    sin(a) sin(theta_i) cos(phi) + cos(a) cos(theta_i) =: A cos(phi) + B, whose
    positive part integrates over phi in closed form: 2 pi B for B >= A, else
    2 (B phi0 + A sin(phi0)) with phi0 = acos(-B / A); the integral over a is
    scipy's quad."""
    from scipy.integrate import quad
    ci = float(cos_i)
    si = np.sqrt(max(0.0, 1.0 - ci * ci))

    def ring(a):
        A, B = np.sin(a) * si, np.cos(a) * ci
        if B >= A:
            return 2 * np.pi * B
        p0 = np.arccos(-B / A)
        return 2 * (B * p0 + A * np.sin(p0))

    lobe, _ = quad(lambda a: np.cos(a) ** n * np.sin(a) * ring(a), 0.0, np.pi / 2, epsabs=1e-12, epsrel=1e-12,
                   limit=200)
    return rho + ks * (n + 2) / (2 * np.pi) * lobe


def test_phong_albedo_quadrature_cross_check():
    """The closed-form ring integral of _phong_albedo against a plain 2-D
    quadrature over the hemisphere, and the normal-incidence closed form ks + rho
    (int cos^(n+1) over the hemisphere = 2 pi / (n + 2))."""
    from scipy.integrate import dblquad
    ks, n, rho = 0.6, 5.0, 0.1
    ci = np.cos(0.7)
    wi = np.array([np.sin(0.7), 0.0, ci])
    R = np.array([-wi[0], -wi[1], wi[2]])

    def f(phi, th):
        wo = np.array([np.sin(th) * np.cos(phi), np.sin(th) * np.sin(phi), np.cos(th)])
        al = max(0.0, float(wo @ R))
        return (ks * (n + 2) / (2 * np.pi) * al ** n + rho / np.pi) * wo[2] * np.sin(th)

    want, _ = dblquad(f, 0.0, np.pi / 2, 0.0, 2 * np.pi, epsabs=1e-9, epsrel=1e-9)
    np.testing.assert_allclose(_phong_albedo(ci, ks, n, rho), want, rtol=1e-7)
    np.testing.assert_allclose(_phong_albedo(1.0, 0.3, 30.0, 0.5), 0.8, rtol=1e-10)


@pytest.mark.parametrize("rho,ks,n", [(0.5, 0.3, 30.0), (0.0, 0.6, 5.0)])
def test_phong_albedo_known_answer(oracle, scenes, rho, ks, n):
    """The oracle's Phong bounce against the directional albedo by quadrature,
    in the form of test_li_oracle.py::test_plastic_albedo_known_answer: the box
    whose far face is Phong and whose other faces are black emitters (Le = 1),
    one scatter (maxDepth 2) -- a pixel's expected radiance is the albedo at its
    camera ray's incidence angle -- and that test's acceptance rule.  (rho 0, ks
    0.6, n 5): the specular sampling weight is exactly 1, only the specular
    lobe is sampled and the part of it below the horizon is void."""
    d = _furnace(0.0, 1.0, w=24, h=16)
    bp, rho3 = scenes.phong_params((rho,) * 3, (ks,) * 3, n)
    np.testing.assert_array_equal(rho3, np.float32([rho] * 3))      # (no energy rescaling: ks + rho <= 1)
    far = 5
    d["bsdf"] = np.zeros(6, np.int32)
    d["bsdf"][far] = 1
    d["reflectance"] = np.float32([0.0, 0.0, 0.0, *rho3])
    d["bsdf_params"] = np.concatenate([np.zeros(8, np.float32), bp])
    d["emitter"] = np.zeros(6, np.int32)
    d["emitter"][far] = -1
    aabb = np.float32([[0, 0, 0, 1, 1, 1]])
    child = np.int32([[-1, -1]])
    spp = 256
    r = oracle.li_render(d, aabb, child, spp=spp, max_depth=2, rr_depth=2, V=1, seed=5, threads=4)
    W, H = d["width"], d["height"]
    tanx = np.tan(np.radians(35.0))
    sx = (np.arange(W) + 0.5) / W
    sy = (np.arange(H) + 0.5) / H
    lx = (1 - 2 * sx)[None, :] * tanx
    ly = (1 - 2 * sy)[:, None] * tanx / (W / H)
    cos_i = 1 / np.sqrt(lx ** 2 + ly ** 2 + 1)
    cache = {}
    want = np.array([cache.setdefault(round(c, 12), _phong_albedo(c, float(bp[1]), float(bp[4]), float(rho3[0])))
                     for c in cos_i.reshape(-1)]).reshape(H, W)
    img = r["image"][0]
    var = (r["image_sqr"][0] - img ** 2) / spp                         # per-pixel variance of the mean
    err = abs(img.mean() - want.mean())
    sig = np.sqrt(var.sum()) / img.size
    print("phong albedo", img.mean(), want.mean(), sig)
    assert err <= 4 * sig + 2e-4, (img.mean(), want.mean(), sig)
    if rho == 0.0:
        assert bp[5] == 1.0 and 0 < (r["nv"] == 1).mean() < 1            # void specular samples save no vertex
    else:
        assert 0 < bp[5] < 1 and (r["nv"] == 1).mean() > 0.9


def test_threads_do_not_change_results_phong(oracle, scenes):
    d = _furnace(0.0, 1.0)
    bp, rho = scenes.phong_params((0.5, 0.3, 0.1), (0.3, 0.4, 0.2), 8.0)
    d["reflectance"] = rho
    d["bsdf_params"] = bp
    aabb = np.float32([[0, 0, 0, 1, 1, 1]])
    child = np.int32([[-1, -1]])
    a = oracle.li_render(d, aabb, child, spp=2, max_depth=10, rr_depth=3, V=9, seed=3, threads=1)
    b = oracle.li_render(d, aabb, child, spp=2, max_depth=10, rr_depth=3, V=9, seed=3, threads=5)
    for k in ("image", "image_sqr", "rec", "nv", "hit_bsdf"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert (a["nv"] < 9).any() and (a["nv"] > 3).any()
    # a Phong scene is not rendered as a diffuse one
    d2 = dict(d)
    del d2["bsdf_params"]
    c = oracle.li_render(d2, aabb, child, spp=2, max_depth=10, rr_depth=3, V=9, seed=3, threads=5)
    assert not np.array_equal(a["rec"], c["rec"])
