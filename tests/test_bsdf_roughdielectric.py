"""CPU: the rough dielectric BSDF (bsdf kind 4, csrc/bsdf_roughdielectric.h)
behind sdmm_bsdf_roughdielectric_host against a restatement of
roughdielectric.cpp:317-662 (isotropic Beckmann, sampleVisible = false, both
components, ERadiance) in numpy float64; its albedo known answer; scene
validation and the shipped synthetic SDMM5.

The tests print their figures; DESIGN.md section 10 holds the last ones."""
import numpy as np
import pytest

ETA = 1.5046


# ---- roughdielectric.cpp in numpy, any float dtype, vectorised over rows ----
def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _fresnel(ci, eta):
    """fresnelDielectricExt (util.cpp:651-681): (F, cosThetaT, 1 - sin^2 scale^2)."""
    dt = ci.dtype.type
    scale = np.where(ci > 0, dt(1) / eta, eta)
    ct2 = dt(1) - (dt(1) - ci * ci) * (scale * scale)
    tir = ct2 <= 0
    a, ct = np.abs(ci), np.sqrt(np.where(tir, dt(1), ct2))
    rs = (a - eta * ct) / (a + eta * ct)
    rp = (eta * a - ct) / (eta * a + ct)
    F = np.where(tir, dt(1), dt(0.5) * (rs * rs + rp * rp))
    return F, np.where(tir, dt(0), np.where(ci > 0, -ct, ct)), ct2


def _beckmann_d(m, alpha):
    """microfacet.h:191-233: (D, the Beckmann exponent tan^2 / alpha^2)."""
    dt = m.dtype.type
    up = m[..., 2] > 0
    c2 = np.where(up, m[..., 2] * m[..., 2], dt(1))
    ex = ((m[..., 0] * m[..., 0]) / (alpha * alpha) + (m[..., 1] * m[..., 1]) / (alpha * alpha)) / c2
    r = np.exp(-ex) / (dt(np.pi) * alpha * alpha * c2 * c2)
    r = np.where(r * m[..., 2] < dt(1e-20), dt(0), r)
    return np.where(up, r, dt(0)), ex


def _g1(v, m, alpha):
    """smithG1 (microfacet.h:477-518)."""
    dt = v.dtype.type
    tmp = dt(1) - v[..., 2] * v[..., 2]
    tan_t = np.where(tmp <= 0, dt(0), np.abs(np.sqrt(np.maximum(tmp, dt(0))) / v[..., 2]))
    with np.errstate(divide="ignore"):
        a = dt(1) / (alpha * tan_t)
    a2 = a * a
    with np.errstate(invalid="ignore"):
        g = (dt(3.535) * a + dt(2.181) * a2) / (dt(1) + dt(2.276) * a + dt(2.577) * a2)
    g = np.where((tan_t == 0) | (a >= dt(1.6)), dt(1), g)
    return np.where(_dot(v, m) * v[..., 2] <= 0, dt(0), g)


def _sample_alpha(alpha, cos_i):
    dt = cos_i.dtype.type
    return alpha * (dt(1.2) - dt(0.2) * np.sqrt(np.abs(cos_i)))


def rd_eval_pdf(wi, wo, eta, alpha, R, T, dtype=np.float64):
    """eval (:317-395, ERadiance) and pdf (:397-469): f (n, 3), pdf (n,) and
    the float quantities the exemptions are decided on."""
    dt = dtype
    wi, wo = np.asarray(wi, dt), np.asarray(wo, dt)
    eta, alpha = dt(eta), dt(alpha)
    R, T = np.asarray(R, dt), np.asarray(T, dt)
    inv_eta = dt(1) / eta
    reflect = wi[..., 2] * wo[..., 2] > 0
    e = np.where(wi[..., 2] > 0, eta, inv_eta)
    hs = np.where(reflect[..., None], wo + wi, wi + wo * e[..., None])
    H = hs * (dt(1) / np.sqrt(_dot(hs, hs)))[..., None]
    H = H * np.copysign(dt(1), H[..., 2])[..., None]
    wi_h, wo_h = _dot(wi, H), _dot(wo, H)
    D, ex = _beckmann_d(H, alpha)
    F, _, ct2 = _fresnel(wi_h, eta)
    G = _g1(wi, H, alpha) * _g1(wo, H, alpha)
    sd = wi_h + e * wo_h
    with np.errstate(divide="ignore", invalid="ignore"):
        vr = F * D * G / (dt(4) * np.abs(wi[..., 2]))
        vt = ((dt(1) - F) * D * G * e * e * wi_h * wo_h) / (wi[..., 2] * sd * sd)
        factor = np.where(wi[..., 2] > 0, inv_eta, eta)
        f = np.where(reflect[..., None], R * vr[..., None], T * np.abs(vt * factor * factor)[..., None])
        f = np.where(((D == 0) | (wi[..., 2] == 0))[..., None], dt(0), f)
        dwh = np.where(reflect, dt(1) / (dt(4) * wo_h), (e * e * wo_h) / (sd * sd))
        Ds, _ = _beckmann_d(H, _sample_alpha(alpha, wi[..., 2]))
        prob = Ds * H[..., 2] * np.where(reflect, F, dt(1) - F)
        pdf = np.where(wi[..., 2] == 0, dt(0), np.abs(prob * dwh))
    aux = {"exponent": ex, "ct2": ct2, "wi_h": wi_h, "wo_h": wo_h, "e": e, "reflect": reflect}
    return f, pdf, aux


def rd_sample(wi, u, eta, alpha, R, T, dtype=np.float64):
    """sample(bRec, pdf, sample) (:560-662), u[:, 2] for sampler->next1D():
    wo, weight (n, 3), pdf, bRec.eta, reflected?, void?, F, sin theta_m,
    cosThetaT."""
    dt = dtype
    wi, u = np.asarray(wi, dt), np.asarray(u, dt)
    eta, alpha = dt(eta), dt(alpha)
    R, T = np.asarray(R, dt), np.asarray(T, dt)
    inv_eta = dt(1) / eta
    a_s = _sample_alpha(alpha, wi[..., 2])
    phi = (dt(2) * dt(np.pi)) * u[..., 1]
    tan2 = a_s * a_s * -np.log(dt(1) - u[..., 0])
    ct = dt(1) / np.sqrt(dt(1) + tan2)
    mpdf = (dt(1) - u[..., 0]) / (dt(np.pi) * a_s * a_s * ct * ct * ct)
    mpdf = np.where(mpdf < dt(1e-20), dt(0), mpdf)
    st = np.sqrt(np.maximum(dt(0), dt(1) - ct * ct))
    m = np.stack([st * np.cos(phi), st * np.sin(phi), ct], -1)
    dm = _dot(wi, m)
    F, cos_t, _ = _fresnel(dm, eta)
    refl = u[..., 2] <= F
    wo_r = (dt(2) * dm)[..., None] * m - wi
    er = np.where(cos_t < 0, inv_eta, eta)
    wo_t = m * (dm * er + cos_t)[..., None] - wi * er[..., None]
    wo = np.where(refl[..., None], wo_r, wo_t)
    crossed = np.where(refl, dt(1), np.where(cos_t < 0, eta, inv_eta))
    side = wi[..., 2] * wo[..., 2]
    void = (mpdf == 0) | np.where(refl, side <= 0, (cos_t == 0) | (side >= 0)) | (wi[..., 2] == 0)
    factor = np.where(cos_t < 0, inv_eta, eta)
    wo_m = _dot(wo, m)
    sd = dm + crossed * wo_m
    with np.errstate(divide="ignore", invalid="ignore"):
        dwh = np.where(refl, dt(1) / (dt(4) * wo_m), (crossed * crossed * wo_m) / (sd * sd))
        D, _ = _beckmann_d(m, alpha)
        G = _g1(wi, m, alpha) * _g1(wo, m, alpha)
        scal = np.abs(D * G * dm / (mpdf * wi[..., 2]))
        w = np.where(refl[..., None], R, T * (factor * factor)[..., None]) * scal[..., None]
        pdf = np.abs(mpdf * np.where(refl, F, dt(1) - F) * dwh)
    w = np.where(void[..., None], dt(0), w)
    pdf = np.where(void, dt(0), pdf)
    crossed = np.where(void, dt(1), crossed)
    return wo, w, pdf, crossed, refl, void, F, st, cos_t


def albedo64(cos_i, eta, alpha, R, T, se_target):
    """The integral of the float64 eval (it holds |cos theta_o|) over the whole
    sphere of wo at wi = (sin, 0, cos theta_i), per channel: Gauss-Legendre in
    cos theta_o on each hemisphere (eval is discontinuous across the
    equator), the periodic trapezoid in phi; refined until it changes by less
    than se_target / 4."""
    wi = np.array([np.sqrt(1 - cos_i * cos_i), 0.0, cos_i])
    prev, n = None, 96
    while True:
        x, wx = np.polynomial.legendre.leggauss(n)
        phi = (np.arange(2 * n) + 0.5) * (np.pi / n)
        tot = np.zeros(3)
        for lo, hi in ((-1.0, 0.0), (0.0, 1.0)):
            z = 0.5 * (hi - lo) * x + 0.5 * (hi + lo)
            Z, P = np.meshgrid(z, phi, indexing="ij")
            s = np.sqrt(1 - Z * Z)
            wo = np.stack([s * np.cos(P), s * np.sin(P), Z], -1)
            f, _, _ = rd_eval_pdf(np.broadcast_to(wi, wo.shape), wo, eta, alpha, R, T)
            tot += np.einsum("i,ijc->c", 0.5 * (hi - lo) * wx, f) * (np.pi / n)
        if prev is not None and np.max(np.abs(tot - prev)) < 0.25 * se_target:
            return tot
        assert n < 3000, "albedo quadrature does not converge"
        prev, n = tot, 2 * n


def params(scenes, alpha, R=(1.0, 1.0, 1.0), T=(1.0, 1.0, 1.0), eta=ETA):
    return scenes.dielectric_params(R, T, int_ior=eta, ext_ior=1.0, alpha=alpha)


class HostBsdf:
    """sdmm_bsdf_roughdielectric_host with reused buffers (the tests make 10^5 calls)."""

    def __init__(self, pkg, bp, st):
        self.fn = pkg.lib().sdmm_bsdf_roughdielectric_host
        self.bp, self.st = np.ascontiguousarray(bp, np.float32), np.ascontiguousarray(st, np.float32)
        self.wi, self.u = np.zeros(3, np.float32), np.zeros(3, np.float32)
        self.wo, self.val, self.out = np.zeros(3, np.float32), np.zeros(3, np.float32), np.zeros(2, np.float32)
        self.ptr = [a.ctypes.data for a in (self.bp, self.st, self.wi, self.u, self.wo, self.val)]
        self.ptr += [self.out.ctypes.data, self.out.ctypes.data + 4]

    def sample(self, wi, u):
        self.wi[:], self.u[:] = wi, u
        assert self.fn(*self.ptr) == 0
        return self.wo.copy(), self.val.copy(), float(self.out[0]), float(self.out[1])

    def eval(self, wi, wo):
        self.wi[:], self.wo[:] = wi, wo
        p = self.ptr
        assert self.fn(p[0], p[1], p[2], None, p[4], p[5], p[6], p[7]) == 0
        return self.val.copy(), float(self.out[0]), float(self.out[1])


def sphere_wi(rng, n, zmin=0.02):
    """Unit float32 directions on the whole sphere, |z| >= zmin."""
    out = []
    while len(out) < n:
        v = rng.normal(size=3)
        v /= np.linalg.norm(v)
        if abs(v[2]) >= zmin:
            out.append(v)
    w = np.float32(out)
    return (w / np.linalg.norm(w.astype(np.float64), axis=1)[:, None]).astype(np.float32)


def _exempt(aux, transmit):
    """The three exemptions, decided on float64 quantities only."""
    e1 = aux["exponent"] > 20
    e2 = np.abs(aux["ct2"]) < 1e-3
    a, b = aux["wi_h"], aux["e"] * aux["wo_h"]
    e3 = transmit & (np.abs(a + b) < 1e-2 * (np.abs(a) + np.abs(b)))
    return e1 | e2 | e3


def _rel(got, ref):
    return np.abs(got - ref) / np.maximum(np.abs(ref), 1e-30)


def check_matches_float64(make_bsdf, scenes, alpha, who="host"):
    """The body of test_host_matches_float64 for any implementation with
    HostBsdf's sample / eval (make_bsdf(bp, st)); returns the exempt share.

    wo, value, pdf and eta_out of the host's sample against the float64
    sample of the same (wi, u), and its eval-mode call at the wo it returned
    against the float64 eval / pdf at that same float32 wo: rtol 1e-5 outside
    the three exempt conditions (<= 3 % of the pairs); at alpha 0.5 the bound
    is 4x the worst non-exempt error of the same formulas in plain numpy
    float32, never below 1e-5.  Each comparison gives both sides the same
    inputs.  (Judging the sample's value and pdf against the float64 eval / pdf
    at the float32 wo, as the Phong host test does, is unsound here: rounding
    an exact wo to float32 alone moves them by up to 6e-5 at grazing
    directions, so no implementation that returns a float32 wo could pass.)

    wo: atol 4e-6 + 5e-7 / sin(theta_m), and on transmission + 1e-6 / |cos
    theta_t| -- what a float32 evaluation may lose to the cancellations in
    sqrt(1 - cos^2 theta_m) and in cosThetaT; the library's double arithmetic
    stays far inside it.

    Plain float32 does not reach rtol 1e-5 on these draws (numpy float32, worst
    non-exempt error: 2.2e-3 / 6.0e-4 / 7.5e-4 at alpha 0.05 / 0.2 / 0.5 -- the
    cancellation of sin theta_m against the Beckmann exponent, cosThetaT near
    the critical angle, wo.z and wo.m at grazing directions), which is why
    csrc/bsdf_roughdielectric.h computes in double between its float inputs
    and outputs.  The figures of a run are printed; DESIGN.md section 10 holds
    the last ones."""
    rng = np.random.default_rng(1234 + int(alpha * 100))
    n = 6000
    bp, st = params(scenes, alpha, (0.9, 0.8, 0.7), (0.6, 0.95, 0.85))
    R, T = bp[1:4].astype(np.float64), st.astype(np.float64)
    eta64, alpha64 = float(bp[4]), float(bp[6])
    W = sphere_wi(rng, n)
    U = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    host = make_bsdf(bp, st)
    got = [host.sample(w, u) for w, u in zip(W, U)]
    wo = np.float32([g[0] for g in got])
    val = np.float32([g[1] for g in got])
    pdf = np.float32([g[2] for g in got])
    eo = np.float32([g[3] for g in got])
    ev = [host.eval(w, o) for w, o in zip(W, wo)]
    fe, pe, ee = np.float32([e[0] for e in ev]), np.float32([e[1] for e in ev]), np.float32([e[2] for e in ev])

    wo64, _, _, c64, refl, void, F64, st_m, ct_m = rd_sample(W, U, eta64, alpha64, R, T)
    wo32, w32, p32, _, refl32, void32, _, _, _ = rd_sample(W, U, np.float32(eta64), np.float32(alpha64), R, T,
                                                             np.float32)
    # a lobe choice or a side check may flip in float32 only at a near tie
    lib_void = (pdf == 0) & (val == 0).all(1)
    near = (np.abs(U[:, 2].astype(np.float64) - F64) < 1e-5) | (np.abs(W[:, 2] * wo64[:, 2]) < 1e-5)
    assert ((lib_void == void) | near).all()
    ok = ~void & ~lib_void & (void32 == void) & (refl32 == refl)
    assert (eo[ok] == np.where(refl, 1.0, c64).astype(np.float32)[ok]).all()
    assert (ee[ok] == eo[ok]).all()            # the given-direction reading agrees with sample's
    assert (eo[lib_void] == 1.0).all()

    _, w64, p64, _, _, _, _, _, _ = rd_sample(W, U, eta64, alpha64, R, T)

    def errors(wo_, value, pdf_, f_eval, p_eval):
        """(relative errors of the sample's value and pdf against the float64
        sample of the same u, and of the eval-mode pair against float64 at the
        float32 direction wo_; the exempt rows)"""
        f, p, aux = rd_eval_pdf(W, wo_, eta64, alpha64, R, T)
        with np.errstate(divide="ignore", invalid="ignore"):
            e = np.stack([_rel(value, w64).max(1), _rel(pdf_, p64), _rel(f_eval, f).max(1), _rel(p_eval, p)]).max(0)
        return e, _exempt(aux, ~refl)
    e_lib, ex = errors(wo, val, pdf, fe, pe)
    f32, pe32, _ = rd_eval_pdf(W, wo32, np.float32(eta64), np.float32(alpha64), R, T, np.float32)
    e_32, ex32 = errors(wo32, w32, p32, f32, pe32)
    use = ok & ~ex
    share = float((ok & ex).sum()) / float(ok.sum())
    worst = float(e_lib[use].max())
    worst32 = float(e_32[ok & ~ex32].max())
    bound = 1e-5 if alpha < 0.5 else max(1e-5, 4 * worst32)
    inside = int((W[:, 2] < 0).sum())
    print(f"roughdielectric {who} alpha {alpha}: worst non-exempt rel err {worst:.3g} (bound {bound:.3g}; numpy "
          f"float32 {worst32:.3g}), exempt {100 * share:.2f} %, reflected {int((refl & ok).sum())}, transmitted "
          f"{int((~refl & ok).sum())}, inside {inside}, void {int(lib_void.sum())}")
    wo_tol = 4e-6 + 5e-7 / np.maximum(st_m, 1e-30) + np.where(refl, 0.0, 1e-6 / np.maximum(np.abs(ct_m), 1e-30))
    wo_err = np.abs(wo - wo64).max(1) / wo_tol
    print(f"  wo: worst error / its bound {float(wo_err[use].max()):.3g}")
    assert (wo_err[use] <= 1.0).all()
    assert share <= 0.03
    assert (refl & ok).sum() > 300 and (~refl & ok).sum() > 1000 and inside > 2000 and lib_void.sum() > 5
    assert n - inside > 2000
    assert worst <= bound
    return share


@pytest.mark.parametrize("alpha", [0.05, 0.2, 0.5])
def test_host_matches_float64(pkg, scenes, alpha):
    """check_matches_float64 (above: inputs, tolerances, exemptions) on
    sdmm_bsdf_roughdielectric_host."""
    check_matches_float64(lambda bp, st: HostBsdf(pkg, bp, st), scenes, alpha)


def _threshold(host, wi, u01):
    """The largest 24-bit u2 for which the host's sample reflects (F rounded
    down to the uniform grid), by bisection on the lobe; -1: never."""
    def reflects(k):
        wo, _, _, eta = host.sample(wi, (u01[0], u01[1], np.float32(k) / np.float32(16777216.0)))
        return eta == 1.0 and wo[2] * wi[2] > 0
    if not reflects(0):
        return -1
    lo, hi = 0, 16777215
    if reflects(hi):
        return hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if reflects(mid) else (lo, mid)
    return lo


def test_lobe_split_and_edges(pkg, scenes):
    """Reflection exactly when u2 <= F; eta_out 1 / eta / 1 / eta; wi.z == 0
    is 0; a total internal reflection never transmits."""
    rng = np.random.default_rng(99)
    bp, st = params(scenes, 0.2)
    host = HostBsdf(pkg, bp, st)
    eta, inv_eta = np.float32(bp[4]), np.float32(bp[5])
    n_enter = n_leave = n_thr = 0
    for wi in sphere_wi(rng, 300, 0.3):
        u = rng.uniform(0, 1, 3).astype(np.float32)
        F64 = rd_sample(wi[None], u[None], float(eta), 0.2, np.ones(3), np.ones(3))[6]
        # the microfacet normal does not depend on u2: reflection <=> u2 <= F
        wo_r, v_r, p_r, e_r = host.sample(wi, (u[0], u[1], 0.0))
        if p_r > 0:
            assert e_r == 1.0 and wo_r[2] * wi[2] > 0
            k = _threshold(host, wi, u)
            if 0 <= k < 16777215 and abs(F64[0] - 1) > 1e-3:
                n_thr += 1
                assert abs((k + 0.5) / 16777216.0 - F64[0]) <= 1e-5 * F64[0] + 1.0 / 16777216.0
        wo_t, v_t, p_t, e_t = host.sample(wi, (u[0], u[1], np.float32(1 - 2.0 ** -24)))
        if p_t > 0 and wo_t[2] * wi[2] < 0:
            if wi[2] > 0:
                n_enter += 1
                assert e_t == eta
            else:
                n_leave += 1
                assert e_t == inv_eta
            # the given-direction reading is the same
            assert host.eval(wi, wo_t)[2] == e_t
    assert n_enter > 50 and n_leave > 20 and n_thr > 50
    # wi.z == 0
    wi0 = np.float32([0.6, 0.8, 0.0])
    f, p, _ = host.eval(wi0, np.float32([0.0, 0.6, 0.8]))
    assert p == 0.0 and (f == 0.0).all()
    _, v, p, e = host.sample(wi0, (0.3, 0.3, 0.3))
    assert p == 0.0 and (v == 0.0).all() and e == 1.0
    # inside, well beyond the critical angle (sin = 0.954 > 1 / eta = 0.665),
    # smooth enough that every microfacet sees a total internal reflection
    bp2, st2 = params(scenes, 0.02)
    host2 = HostBsdf(pkg, bp2, st2)
    wi = np.float32([0.9539392, 0.0, -0.3])
    for u in rng.uniform(0, 1, (500, 3)).astype(np.float32):
        u[2] = np.float32(1 - 2.0 ** -24) if u[2] > 0.5 else u[2]
        wo, v, p, e = host2.sample(wi, u)
        assert e == 1.0 and (p == 0.0 or wo[2] < 0)


@pytest.mark.parametrize("RT", [(1.0, 1.0), (1.0, 0.0), (0.0, 1.0)])
@pytest.mark.parametrize("side", [1.0, -1.0])
@pytest.mark.parametrize("theta_deg", [20.0, 60.0])
def test_albedo_known_answer(pkg, scenes, theta_deg, side, RT):
    """The mean of `value` over 2^16 samples equals the quadrature of the
    float64 eval over the whole sphere within 4 standard errors: sample, pdf
    and eval are consistent, the eta^2 factor and the half-vector Jacobian
    included."""
    alpha = 0.3
    bp, st = params(scenes, alpha, (RT[0],) * 3, (RT[1],) * 3)
    host = HostBsdf(pkg, bp, st)
    th = np.radians(theta_deg)
    wi = np.float32([np.sin(th), 0.0, side * np.cos(th)])
    wi = (wi / np.linalg.norm(wi.astype(np.float64))).astype(np.float32)
    rng = np.random.default_rng(int(theta_deg) * 7 + int(side) + int(RT[0] * 2 + RT[1]))
    U = rng.uniform(0, 1, (1 << 16, 3)).astype(np.float32)
    v = np.array([host.sample(wi, u)[1][0] for u in U], np.float64)
    mean, se = float(v.mean()), float(v.std(ddof=1) / np.sqrt(v.size))
    ref = albedo64(float(wi[2]), float(bp[4]), alpha, (RT[0],) * 3, (RT[1],) * 3, se)[0]
    print(f"albedo theta {theta_deg} side {side:+.0f} R {RT[0]} T {RT[1]}: mean {mean:.5f} +- {se:.5f}, "
          f"quadrature {ref:.5f} ({abs(mean - ref) / se:.2f} sigma)")
    assert se > 0 and abs(mean - ref) < 4 * se


def test_scene_rejects_invalid_dielectric(pkg, scenes):
    def scene_with(**kw):
        return scenes.cornell_box(32, 18, dielectric=("TallBox",), **kw)
    i = list(scenes._BSDFS).index("TallBox")
    for eta, inv in ((1.0, 1.0), (0.0, 1.0), (-1.5, -1 / 1.5)):
        desc = scene_with()
        desc["bsdf_params"][8 * i + 4] = eta
        desc["bsdf_params"][8 * i + 5] = inv
        with pytest.raises(pkg.SDMMError, match="invalid bsdf_params"):
            pkg.Scene(desc)
    desc = scene_with()
    desc["learned_models_nd"][i] = scenes.load_learned()           # C = 2
    with pytest.raises(pkg.SDMMError, match="C = 3"):
        pkg.Scene(desc)
    with pytest.raises(ValueError):
        scenes.dielectric_params(int_ior=1.5, ext_ior=1.5)


def test_shipped_model(pkg, scenes, tmp_path):
    """dielectric_4c.sdmm5.json round-trips; pruned to 2 without a forced lobe
    it gives two lobes for theta_i across (0, pi / 2), the heaviest below the
    surface at normal incidence."""
    L = pkg.LearnedBSDFND.load_json(scenes.LEARNED_DIELECTRIC)
    assert L.C == 3 and L.M == 4
    for a, b in zip(L.arrays(), scenes.load_learned_nd(scenes.LEARNED_DIELECTRIC)):
        np.testing.assert_array_equal(a, b)
    L.save_json(tmp_path / "d.sdmm5.json")
    assert (tmp_path / "d.sdmm5.json").read_text() == scenes.LEARNED_DIELECTRIC.read_text()
    assert (L.means[:, 5] < 0).sum() == 2 and (L.means[:, 5] > 0).sum() == 2
    bp, _ = scenes.dielectric_params(alpha=0.2)
    for th in np.linspace(0.02, np.pi / 2 - 0.02, 24):
        w, m, c = L.conditional([bp[6], bp[4]], np.float32([np.sin(th), 0.0, np.cos(th)]), keep=2, force=-1)
        assert len(w) == 2 and np.isfinite(m).all() and np.isfinite(c).all() and abs(w.sum() - 1) < 1e-5
    w, m, _ = L.conditional([bp[6], bp[4]], np.float32([0.0, 0.0, 1.0]), keep=2, force=-1)
    assert m[np.argmax(w), 2] < 0
    # a hit from inside has no learned BSDF (roughdielectric.cpp:199)
    assert len(L.conditional([bp[6], bp[4]], np.float32([0.6, 0.0, -0.8]), keep=2, force=-1)[0]) == 0
