"""Learned BSDFs over a C-dimensional condition (sdmm_learned_bsdf,
csrc/learned_bsdf.h learned_conditional<C>) and the Phong BSDF of the device
Li (csrc/bsdf_phong.h), on the host -- the same code the device runs.

The reference's SDMM5 materials (bsdf.h:316-324): Phong conditions on
(theta_i, specWeight, log exponent) with create_conditional_pruned(..., 2,
diffuse_component = 1) (phong.cpp:75-90), rough dielectric / plastic on
(theta_i, alpha, eta); Blend uses the unpruned create_conditional on its SDMM4
(blendbsdf.cpp:87-99).  sdmm-lib is absent, so the semantics are this
library's stated reading; pinned here: C = 2 against the oracle-pinned SDMM4
path bitwise, C = 3 by reduction to it and against float64 known answers, the
selection rules, the JSON form, and Phong::sample / eval / pdf against a
float64 restatement of phong.cpp:171-289."""
import ctypes as C

import numpy as np
import pytest

from test_learned_bsdf import _coords, _wi


def _embed(model, mean2=0.37, var2=0.09):
    """The SDMM4 `model` with an independent third condition coordinate: the
    same mean and variance in every component, zero cross-covariance."""
    w, mu, cv = model
    M = len(w)
    mu5 = np.concatenate([mu[:, :2], np.full((M, 1), mean2, np.float32), mu[:, 2:]], 1)
    cv5 = np.zeros((M, 5, 5), np.float32)
    keep = [0, 1, 3, 4]
    cv5[np.ix_(range(M), keep, keep)] = cv.reshape(M, 4, 4)
    cv5[:, 2, 2] = var2
    return w, mu5.astype(np.float32), cv5.reshape(M, 25)


@pytest.mark.parametrize("keep", [1, 2, 4])
def test_c2_equals_pinned_sdmm4_path_bitwise(pkg, oracle, scenes, keep):
    m = scenes.load_learned()
    L4, L = pkg.LearnedBSDF(*m), pkg.LearnedBSDFND(*m)
    assert L.C == 2
    W = _wi(np.random.default_rng(40 + keep), 1500)
    for i, wl in enumerate(W):
        alpha = float((0.03, 0.2, 0.6)[i % 3])
        a = L.conditional([alpha], wl, keep, -1)
        for ref in (L4.conditional(alpha, wl, keep), oracle.learned4_conditional(m, alpha, wl, keep)):
            for x, y in zip(a, ref):
                np.testing.assert_array_equal(x, y)
        assert len(a[0]) == keep


def test_c3_reduces_to_sdmm4(pkg, scenes):
    """An independent third coordinate multiplies every pi' by one factor and
    adds exact zeros to the shift and the Schur complement: the renormalised
    weights agree to rounding, means and covariances bitwise."""
    m = scenes.load_learned()
    L4, L5 = pkg.LearnedBSDF(*m), pkg.LearnedBSDFND(*_embed(m))
    assert L5.C == 3
    W = _wi(np.random.default_rng(5), 600)
    for i, wl in enumerate(W):
        alpha = float((0.03, 0.2, 0.6)[i % 3])
        c2 = float((0.37, -0.2, 0.9, 0.5)[i % 4])
        for keep in (2, 4):
            a = L5.conditional([alpha, c2], wl, keep, -1)
            b = L4.conditional(alpha, wl, keep)
            assert len(a[0]) == len(b[0]) == keep
            np.testing.assert_allclose(a[0], b[0], rtol=1e-6)
            np.testing.assert_array_equal(a[1], b[1])
            np.testing.assert_array_equal(a[2], b[2])


def test_c3_known_answers(pkg):
    """One component with a full 5x5 covariance A A^T (A lower triangular,
    diagonal >= 0.1: well conditioned): weight 1, the mean the exponential map
    of S_dc S_cc^-1 (x - mu_c), the covariance the Schur complement carried by
    parallel transport -- all in float64 here, as
    test_learned_bsdf.py::test_conditional_known_answers does at 4-D, with
    that test's bounds (mean atol 2e-6, covariance rtol 1e-5 / atol 1e-7;
    realised here: mean 9.2e-8, covariance 0.03 of its bound, so they stand)."""
    c0 = np.float64([0.6, 0.3, 3.0])
    mu = np.float32([-np.sin(0.6), 0.0, np.cos(0.6)])
    A = np.float64([[0.3, 0, 0, 0, 0], [0.05, 0.2, 0, 0, 0], [-0.1, 0.15, 0.8, 0, 0],
                    [-0.25, 0.02, 0.05, 0.15, 0], [0.03, -0.01, -0.04, 0.02, 0.12]])
    cov = (A @ A.T).astype(np.float32)
    L = pkg.LearnedBSDFND(np.float32([1.0]), np.float32([[*c0, *mu]]), cov.reshape(1, 25))
    worst_m = worst_c = 0.0
    for th, sw, le in ((0.6, 0.3, 3.0), (0.75, 0.5, 4.0), (0.4, 0.1, 1.5), (0.9, 0.35, 0.0)):
        wl = np.float32([np.sin(th), 0.0, np.cos(th)])   # azimuth 0: rotate_to_wo is the identity
        w, mean, c = L.conditional([sw, le], wl, 2, -1)
        assert len(w) == 1 and w[0] == 1.0
        Cv = cov.astype(np.float64)
        Scc, Sdc, Sdd = Cv[:3, :3], Cv[3:, :3], Cv[3:, 3:]
        th32 = np.float64(np.float32(np.arccos(min(1.0, float(wl[2])))))
        x = np.float64([th32, np.float32(sw), np.float32(le)])
        shift = Sdc @ np.linalg.solve(Scc, x - np.float64(np.float32(c0)))
        T = _coords(mu)
        ln = np.linalg.norm(shift)
        d = np.cos(ln) * mu + (np.sin(ln) / ln if ln > 0 else 1.0) * (shift[0] * T[0] + shift[1] * T[1])
        np.testing.assert_allclose(mean[0], d, atol=2e-6)
        worst_m = max(worst_m, float(np.abs(mean[0] - d).max()))
        cond = Sdd - Sdc @ np.linalg.solve(Scc, Sdc.T)
        if ln > 0:
            u = shift / ln
            u3 = u[0] * T[0] + u[1] * T[1]
            g = (np.cos(ln) - 1) * u3 - np.sin(ln) * T[2]
            E = np.stack([T[0] + u[0] * g, T[1] + u[1] * g])
        else:
            E = T[:2]
        Td = _coords(d / np.linalg.norm(d))
        B = Td[:2] @ E.T
        want = B @ cond @ B.T
        got = np.float64([[c[0, 0], c[0, 1]], [c[0, 2], c[0, 3]]])
        worst_c = max(worst_c, float((np.abs(got - want) / (1e-7 + 1e-5 * np.abs(want))).max()))
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(np.linalg.eigvalsh(got), np.linalg.eigvalsh(cond), rtol=1e-5)
    print(f"c3 known answers: mean err {worst_m:.3g} (bound 2e-6), covariance err / bound {worst_c:.3g}")


def _four(bad_scc=False):
    """Four components told apart by their directions, S_dc = 0; at theta =
    0.5 they rank 0 > 2 > 3 > 1 (component 1 sits far away in theta)."""
    th = [0.5, 1.4, 0.6, 0.8]
    dirs = [[0.0, 0.0, 1.0], [0.6, 0.0, 0.8], [0.0, 0.6, 0.8], [-0.6, 0.0, 0.8]]
    mu = np.float32([[t, 0.4, 2.0, *d] for t, d in zip(th, dirs)])
    cov = np.stack([np.diag(np.float32([0.09, 0.04, 1.0, 0.02, 0.03]))] * 4)
    if bad_scc:
        cov[1, 0, 1] = cov[1, 1, 0] = 0.07          # |rho| > 1: S_cc not PD
    return np.float32([0.25] * 4), mu, cov.reshape(4, 25), np.float32(dirs)


def _which(means, dirs):
    return [int(np.argmin(np.linalg.norm(dirs - m, axis=1))) for m in means]


def test_forced_component_and_unpruned(pkg):
    w, mu, cov, dirs = _four()
    L = pkg.LearnedBSDFND(w, mu, cov)
    wl = np.float32([np.sin(0.5), 0.0, np.cos(0.5)])
    rest = [0.45, 2.3]
    x = np.float64([np.float32(np.arccos(wl[2])), np.float32(0.45), np.float32(2.3)])
    Scc = np.diag(np.float64(np.float32([0.09, 0.04, 1.0])))
    dm = x[None] - mu[:, :3].astype(np.float64)
    pw = 0.25 * np.exp(-0.5 * np.einsum("ki,ij,kj->k", dm, np.linalg.inv(Scc), dm))
    assert list(np.argsort(-pw)) == [0, 2, 3, 1]

    def check(keep, force, want):
        a = L.conditional(rest, wl, keep, force)
        assert _which(a[1], dirs) == want
        np.testing.assert_allclose(a[0], pw[want] / pw[want].sum(), rtol=1e-5)
        np.testing.assert_allclose(a[0].sum(), 1.0, rtol=2e-6)
        return a

    a = check(2, 1, [0, 1])                  # the forced component beside the top one
    assert (np.diff(a[0]) <= 0).all()
    check(2, -1, [0, 2])                     # plain pruning: the top two
    check(3, 1, [0, 2, 1])
    check(1, 1, [1])
    check(2, 0, [0, 2])                      # forcing a component already chosen changes nothing
    check(0, -1, [0, 1, 2, 3])               # unpruned: model order
    check(0, 1, [0, 1, 2, 3])
    # a forced component whose S_cc is not PD has pi' = 0: plain pruning
    Lb = pkg.LearnedBSDFND(*_four(bad_scc=True)[:3])
    b = Lb.conditional(rest, wl, 2, 1)
    assert _which(b[1], dirs) == [0, 2]
    np.testing.assert_allclose(b[0], pw[[0, 2]] / pw[[0, 2]].sum(), rtol=1e-5)
    assert _which(Lb.conditional(rest, wl, 0, -1)[1], dirs) == [0, 2, 3]
    # force >= M: SDMM_E_INVALID
    n = C.c_int()
    out = np.zeros(8 * 8, np.float32)
    rc = pkg.lib().sdmm_learned_conditional(C.byref(L.c), np.float32(rest).ctypes.data, wl.ctypes.data, 2, 4,
                                            C.byref(n), out.ctypes.data, out.ctypes.data, out.ctypes.data)
    assert rc == -1
    with pytest.raises(pkg.SDMMError):
        L.conditional(rest, wl, 2, 4)
    # cos theta_i <= 0: no valid conditional
    assert len(L.conditional(rest, np.float32([0.2, 0.0, -0.9]), 2, 1)[0]) == 0


def test_json_round_trip_and_sdmm4_files(pkg, scenes, tmp_path):
    m5 = _embed(scenes.load_learned())
    L = pkg.LearnedBSDFND(*m5)
    L.save_json(tmp_path / "m.sdmm5.json")
    R = pkg.LearnedBSDFND.load_json(tmp_path / "m.sdmm5.json")
    assert R.C == 3
    for a, b in zip(L.arrays(), R.arrays()):
        np.testing.assert_array_equal(a, b)
    # the shipped files: the Phong model, and the conductor's sdmm4 as C = 2
    P = pkg.LearnedBSDFND.load_json(scenes.LEARNED_PHONG)
    assert P.C == 3 and P.M == 4
    for a, b in zip(P.arrays(), scenes.load_learned_nd()):
        np.testing.assert_array_equal(a, b)
    L2 = pkg.LearnedBSDFND.load_json(scenes.LEARNED_CONDUCTOR)
    assert L2.C == 2
    for a, b in zip(L2.arrays(), scenes.load_learned()):
        np.testing.assert_array_equal(a, b)
    (tmp_path / "bad.json").write_text('{"format": "sdmm-amd.asdmm", "version": 1}')
    with pytest.raises(pkg.SDMMError):
        pkg.LearnedBSDFND.load_json(tmp_path / "bad.json")


# ---- Phong::sample / eval / pdf -------------------------------------------
def _frame64(n):
    """Mitsuba coordinateSystem (s, t) of n."""
    if abs(n[0]) > abs(n[1]):
        inv = 1.0 / np.sqrt(n[0] * n[0] + n[2] * n[2])
        t = np.array([n[2] * inv, 0.0, -n[0] * inv])
    else:
        inv = 1.0 / np.sqrt(n[1] * n[1] + n[2] * n[2])
        t = np.array([0.0, n[2] * inv, -n[1] * inv])
    return np.cross(t, n), t


def _phong_eval_pdf64(bp, rho, wi, wo):
    """phong.cpp:171-230 in float64 (both lobes)."""
    if wi[2] <= 0 or wo[2] <= 0:
        return np.zeros(3), 0.0
    ks, e, ssw = bp[1:4], bp[4], bp[5]
    alpha = np.dot(wo, [-wi[0], -wi[1], wi[2]])
    spec = sprob = 0.0
    if alpha > 0:
        spec = (e + 2) / (2 * np.pi) * alpha ** e
        sprob = alpha ** e * (e + 1) / (2 * np.pi)
    f = (ks * spec + rho / np.pi) * wo[2]
    return f, ssw * sprob + (1 - ssw) * wo[2] / np.pi


def _phong_sample64(bp, wi, u):
    """phong.cpp:232-281 in float64: (wo, specular chosen, sin of the lobe angle / z)."""
    e, ssw = bp[4], bp[5]
    u0, u1 = float(u[0]), float(u[1])
    if u0 <= ssw and ssw > 0:
        u0 /= ssw
        R = np.array([-wi[0], -wi[1], wi[2]])
        sa, ca = np.sqrt(1 - u1 ** (2 / (e + 1))), u1 ** (1 / (e + 1))
        phi = 2 * np.pi * u0
        s, t = _frame64(R)
        return s * (sa * np.cos(phi)) + t * (sa * np.sin(phi)) + R * ca, True, sa
    u0 = (u0 - ssw) / (1 - ssw)
    r1, r2 = 2 * u0 - 1, 2 * u1 - 1
    if r1 == 0 and r2 == 0:
        r, phi = 0.0, 0.0
    elif r1 * r1 > r2 * r2:
        r, phi = r1, (np.pi / 4) * (r2 / r1)
    else:
        r, phi = r2, np.pi / 2 - (r1 / r2) * (np.pi / 4)
    x, y = r * np.cos(phi), r * np.sin(phi)
    z = np.sqrt(max(0.0, 1 - x * x - y * y))
    return np.array([x, y, z if z > 0 else 1e-10]), False, z


def test_phong_host_matches_float64(pkg, scenes):
    """value and pdf against phong.cpp:171-230 in float64 at rtol 1e-5,
    evaluated at the float32 wo the library sampled.  Exponents up to 30 (the
    reference's default): pow(alpha, e) turns the ~1e-7 relative rounding of
    the float32 alpha into e x 1e-7, so rtol 1e-5 resolves e up to about 50.
    The sampled wo against the float64 map of the same u: its error is the
    float32 cancellation in sqrt(1 - p) (p = u1^(2/(e+1)) for the lobe, x^2 +
    y^2 for the cosine hemisphere), at most ~2 ulp(1) / (2 sqrt(1 - p)), beside
    ~1e-6 for the remaining dozen roundings: atol 2e-6 + 3e-7 / sqrt(1 - p)."""
    rng = np.random.default_rng(17)
    mats = [scenes.phong_params((0.5, 0.4, 0.3), (0.3, 0.2, 0.4), 30.0),
            scenes.phong_params((0.725, 0.71, 0.68), (0.4, 0.4, 0.4), 10.0),     # energy-scaled
            scenes.phong_params((0.2, 0.2, 0.2), (0.7, 0.6, 0.5), 1.0),
            scenes.phong_params((0.5, 0.5, 0.5), (0.0, 0.0, 0.0), 30.0)]         # weight 0: always diffuse
    assert np.float32((mats[1][1] + mats[1][0][1:4]).max()) <= 1.0 and mats[3][0][5] == 0.0
    W = _wi(rng, 2000)
    U = rng.uniform(0, 1, (2000, 2)).astype(np.float32)
    n_spec = n_void = 0
    worst = 0.0
    for i, (wi, u) in enumerate(zip(W, U)):
        bp, rho = mats[i % 4]
        if i % 50 == 0:
            u = np.float32([bp[5], u[1]])                 # u0 == weight: still the specular lobe
        wo, value, pdf = pkg.bsdf_phong_host(bp, rho, wi, u=u)
        b64, r64, wi64 = bp.astype(np.float64), rho.astype(np.float64), wi.astype(np.float64)
        wo64, spec, s = _phong_sample64(b64, wi64, u)
        assert spec == (u[0] <= bp[5] and bp[5] > 0)      # the lobe choice splits at the sampling weight
        n_spec += spec
        np.testing.assert_allclose(wo, wo64, rtol=0, atol=2e-6 + 3e-7 / max(s, 1e-30))
        f, p = _phong_eval_pdf64(b64, r64, wi64, wo.astype(np.float64))
        if wo[2] <= 0:
            n_void += 1
            assert spec and pdf == 0.0 and (value == 0.0).all()
            continue
        np.testing.assert_allclose(pdf, p, rtol=1e-5)
        np.testing.assert_allclose(value, f / p, rtol=1e-5, atol=1e-30)
        worst = max(worst, abs(pdf - p) / p, float(np.max(np.abs(value - f / p) / np.maximum(f / p, 1e-30))))
        # eval / pdf of a given direction: the same wo, then an independent one
        for wg in (wo, _wi(rng, 1)[0]):
            _, fe, pe = pkg.bsdf_phong_host(bp, rho, wi, wo=wg)
            f, p = _phong_eval_pdf64(b64, r64, wi64, wg.astype(np.float64))
            np.testing.assert_allclose(pe, p, rtol=1e-5)
            np.testing.assert_allclose(fe, f, rtol=1e-5, atol=1e-30)
        _, fe, pe = pkg.bsdf_phong_host(bp, rho, wi, wo=np.float32([wo[0], wo[1], -wo[2]]))
        assert pe == 0.0 and (fe == 0.0).all()             # wo.z <= 0
    print(f"phong host: worst relative error {worst:.3g} (rtol 1e-5), {n_spec} specular, {n_void} void")
    assert n_spec > 300 and n_void > 0


def test_scene_rejects_invalid_phong_model(pkg, scenes):
    f = list(scenes._BSDFS).index("Floor")
    w, mu, cv = scenes.load_learned_nd()

    def scene_with(model):
        desc = scenes.cornell_box(32, 18, phong=("Floor",))
        desc["learned_models_nd"][f] = model
        return desc

    with pytest.raises(pkg.SDMMError, match="C = 3"):
        pkg.Scene(scene_with(scenes.load_learned()))                    # C = 2
    bad = mu.copy()
    bad[0, 3:] *= 1.5                                                    # a non-unit direction
    with pytest.raises(pkg.SDMMError, match="non-unit direction"):
        pkg.Scene(scene_with((w, bad, cv)))
    with pytest.raises(pkg.SDMMError, match="M >= 2"):
        pkg.Scene(scene_with((w[:1], mu[:1], cv[:1])))                  # M = 1: no component 1 to force
