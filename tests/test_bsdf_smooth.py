"""CPU: the delta-only BSDFs (bsdf kinds 5 and 6, csrc/bsdf_smooth.h) behind
sdmm_bsdf_smooth_host against a restatement of dielectric.cpp:228-333 (both
components, ERadiance) and conductor.cpp:223-285 (a gray conductor) in numpy
float64; the lobe choice at u0 == F; the EDiscrete eval / pdf mode; scene
validation and the scene helpers.

The library computes in double between float inputs and outputs, in the
restatement's order of operations: its outputs are roundings of the float64
values, hence the bound of 1 float32 ulp.  The tests print their figures;
DESIGN.md section 10 holds the last ones."""
import numpy as np
import pytest

ETA = 1.5046
NQ = 4099                                  # a tail in the batch kernel's last workgroup (tests/test_gpu_smooth.py)
BELOW1 = np.float32(1 - 2.0 ** -24)        # the largest float below 1
N_TIE = 30


# ---- dielectric.cpp / conductor.cpp in numpy float64, vectorised over rows ----
def fresnel_dielectric64(ci, eta):
    """fresnelDielectricExt (util.cpp:651-681): (F, cosThetaT, 1 - sin^2 scale^2)."""
    scale = np.where(ci > 0, 1.0 / eta, eta)
    ct2 = 1.0 - (1.0 - ci * ci) * (scale * scale)
    tir = ct2 <= 0
    a, ct = np.abs(ci), np.sqrt(np.where(tir, 1.0, ct2))
    rs = (a - eta * ct) / (a + eta * ct)
    rp = (eta * a - ct) / (eta * a + ct)
    F = np.where(tir, 1.0, 0.5 * (rs * rs + rp * rp))
    return F, np.where(tir, 0.0, np.where(ci > 0, -ct, ct)), ct2


def fresnel_conductor64(ci, eta, k):
    """fresnelConductorExact (util.cpp:739-761) for a gray conductor."""
    ci2 = ci * ci
    si2 = 1.0 - ci2
    si4 = si2 * si2
    t1 = eta * eta - k * k - si2
    a2pb2 = np.sqrt(np.maximum(0.0, t1 * t1 + k * k * eta * eta * 4.0))
    a = np.sqrt(np.maximum(0.0, (a2pb2 + t1) * 0.5))
    term1, term2 = a2pb2 + ci2, a * (2.0 * ci)
    rs2 = (term1 - term2) / (term1 + term2)
    term3, term4 = a2pb2 * ci2 + si4, term2 * si2
    rp2 = rs2 * (term3 - term4) / (term3 + term4)
    return 0.5 * (rp2 + rs2)


def dielectric_sample64(wi, u0, bp, T):
    """SmoothDielectric::sample(bRec, pdf, sample) (:277-308) at sample.x = u0
    from the float32 parameters bp (eta, and 1 / eta as the plugin stores it):
    dict of wo, weight (n, 3), pdf, bRec.eta, reflected?, F, cosThetaT and the
    two margins the exemptions are decided on.  wi.z == 0: weight 0, pdf 0."""
    wi, u0 = np.asarray(wi, np.float64), np.asarray(u0, np.float64)
    eta, inv_eta = float(bp[4]), float(bp[5])
    R, T = np.asarray(bp[1:4], np.float64), np.asarray(T, np.float64)
    F, cos_t, ct2 = fresnel_dielectric64(wi[:, 2], eta)
    refl = u0 <= F
    factor = np.where(cos_t < 0, inv_eta, eta)
    wo = np.where(refl[:, None], np.stack([-wi[:, 0], -wi[:, 1], wi[:, 2]], 1),
                  np.stack([-factor * wi[:, 0], -factor * wi[:, 1], cos_t], 1))
    w = np.where(refl[:, None], R[None], T[None] * (factor * factor)[:, None])
    pdf = np.where(refl, F, 1.0 - F)
    crossed = np.where(refl, 1.0, np.where(cos_t < 0, eta, inv_eta))
    void = wi[:, 2] == 0
    wo = np.where(void[:, None], np.array([0.0, 0.0, 1.0]), wo)
    return {"wo": wo, "w": np.where(void[:, None], 0.0, w), "pdf": np.where(void, 0.0, pdf),
            "eta": np.where(void, 1.0, crossed), "refl": refl, "F": F, "cos_t": cos_t, "void": void,
            "margin_u": np.abs(u0 - F), "margin_ct2": np.abs(ct2)}


def conductor_sample64(wi, bp):
    """SmoothConductor::sample (:270-285): wo, weight, pdf (eta is 1)."""
    wi = np.asarray(wi, np.float64)
    R = np.asarray(bp[1:4], np.float64)
    up = wi[:, 2] > 0
    fr = fresnel_conductor64(np.where(up, wi[:, 2], 1.0), float(bp[4]), float(bp[5]))
    wo = np.where(up[:, None], np.stack([-wi[:, 0], -wi[:, 1], wi[:, 2]], 1), np.array([0.0, 0.0, 1.0]))
    return {"wo": wo, "w": np.where(up[:, None], R[None] * fr[:, None], 0.0), "pdf": np.where(up, 1.0, 0.0),
            "void": ~up}


def ulps(got, ref64):
    """|got - float32(ref64)| in float32 ulps of the reference."""
    ref = np.asarray(ref64, np.float64).astype(np.float32)
    sp = np.spacing(np.maximum(np.abs(ref), np.float32(2.0 ** -126)))
    return np.abs(np.asarray(got, np.float32).astype(np.float64) - ref.astype(np.float64)) / sp.astype(np.float64)


class HostSmooth:
    """sdmm_bsdf_smooth_host with reused buffers."""

    def __init__(self, pkg, bp, st=None):
        self.fn = pkg.lib().sdmm_bsdf_smooth_host
        self.bp = np.ascontiguousarray(bp, np.float32)
        self.st = np.zeros(3, np.float32) if st is None else np.ascontiguousarray(st, np.float32)
        self.wi, self.u = np.zeros(3, np.float32), np.zeros(2, np.float32)
        self.wo, self.val, self.out = np.zeros(3, np.float32), np.zeros(3, np.float32), np.zeros(2, np.float32)
        self.ptr = [a.ctypes.data for a in (self.bp, self.st, self.wi, self.u, self.wo, self.val)]
        self.ptr += [self.out.ctypes.data, self.out.ctypes.data + 4]

    def sample(self, wi, u0):
        self.wi[:], self.u[:] = wi, (u0, 0.5)
        assert self.fn(*self.ptr) == 0
        return self.wo.copy(), self.val.copy(), np.float32(self.out[0]), np.float32(self.out[1])

    def eval(self, wi, wo):
        self.wi[:], self.wo[:] = wi, wo
        p = self.ptr
        assert self.fn(p[0], p[1], p[2], None, p[4], p[5], p[6], p[7]) == 0
        return self.val.copy(), np.float32(self.out[0]), np.float32(self.out[1])

    def sample_rows(self, W, U0):
        """(wo, value, pdf, eta) stacked as (n, 8) float32."""
        return np.float32([np.concatenate([(r := self.sample(w, u))[0], r[1], [r[2], r[3]]]) for w, u in zip(W, U0)])


def sphere_wi(rng, n):
    """Unit float32 directions on the whole sphere."""
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    w = v.astype(np.float32)
    return (w / np.linalg.norm(w.astype(np.float64), axis=1)[:, None]).astype(np.float32)


def glass_params(scenes, R=(0.9, 0.8, 0.7), T=(0.6, 0.95, 0.85), eta=ETA):
    return scenes.smooth_dielectric_params(R, T, int_ior=eta, ext_ior=1.0)


def host_F(host, wi):
    """The largest float32 u0 whose sample reflects (the library's F rounded
    down to a float), by bisection over the bit patterns; None: it never
    transmits (a total internal reflection) or never reflects."""
    def reflects(bits):
        return host.sample(wi, np.uint32(bits).view(np.float32))[3] == 1.0
    hi = int(BELOW1.view(np.uint32))
    if not reflects(0) or reflects(hi):
        return None
    lo = 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if reflects(mid) else (lo, mid)
    return np.uint32(lo).view(np.float32)


def edge_rows(pkg, scenes):
    """The inputs of the host and of the batch test: (bp, st, host, W, U0, tie)
    -- NQ rows of wi over the whole sphere and the lobe uniform, with the edge
    rows placed by hand: wi.z of 0 and +-1e-4, inside hits on both sides of
    the critical angle, u0 of 0 and of the largest float below 1, u0 == F (the
    largest float not above it: even rows) and the next float above it (odd
    rows) for rows 100 .. 100 + N_TIE; tie: those rows' indices."""
    rng = np.random.default_rng(4099)
    bp, st = glass_params(scenes)
    host = HostSmooth(pkg, bp, st)
    W = sphere_wi(rng, NQ)
    U0 = rng.uniform(0, 1, NQ).astype(np.float32)
    W[0] = (0.6, 0.8, 0.0)                                 # wi.z = 0 exactly
    W[1] = (0.6, 0.8, 1e-4)
    W[2] = (0.6, 0.8, -1e-4)
    crit = 1.0 / float(bp[4])                              # sin of the critical angle
    for i in range(3, 40):                                 # inside: beyond the critical angle, then just within it
        s = rng.uniform(crit + 1e-3, 0.999) if i < 22 else rng.uniform(crit - 0.05, crit - 1e-3)
        W[i] = (s, 0.0, -np.sqrt(1 - s * s))
    U0[22:40] = BELOW1                                     # (within the critical angle: these transmit)
    U0[40:60] = 0.0
    U0[60:80] = BELOW1
    tie = []
    for i in range(100, 100 + N_TIE):
        F = host_F(host, W[i])
        if F is not None:
            U0[i] = F if i % 2 == 0 else np.nextafter(F, np.float32(2))
            tie.append(i)
    assert len(tie) > 10 and (W[:, 2] < 0).sum() > 1500 and (W[:, 2] > 0).sum() > 1500
    return bp, st, host, W, U0, tie


def test_dielectric_host_matches_float64(pkg, scenes):
    """wo, weight and pdf within 1 float32 ulp of the float64 restatement,
    eta_out exactly; rows whose float64 |u0 - F| or |1 - sin^2 scale^2| is
    below 1e-6 may take the other branch (at most 1 % of the rows)."""
    bp, st, host, W, U0, tie = edge_rows(pkg, scenes)
    got = host.sample_rows(W, U0)
    ref = dielectric_sample64(W, U0, bp, st)
    exempt = (ref["margin_u"] < 1e-6) | (ref["margin_ct2"] < 1e-6)
    share = float(exempt.mean())
    use = ~exempt
    e_wo = ulps(got[:, :3], ref["wo"])[use].max()
    e_w = ulps(got[:, 3:6], ref["w"])[use].max()
    e_p = ulps(got[:, 6], ref["pdf"])[use].max()
    n_t = int((~ref["refl"] & use).sum())
    print(f"smooth dielectric host: worst ulp wo {e_wo:.3g}, weight {e_w:.3g}, pdf {e_p:.3g}; exempt {int(exempt.sum())} "
          f"of {NQ} ({100 * share:.2f} %), {len(tie)} tie rows, transmitted {n_t}, inside "
          f"{int((W[:, 2] < 0).sum())}, total reflections {int((ref['cos_t'] == 0).sum())}")
    assert share <= 0.01
    assert max(e_wo, e_w, e_p) <= 1.0
    assert (got[use, 7] == ref["eta"].astype(np.float32)[use]).all()
    # both lobes from both sides, and both crossed indices
    assert n_t > 1500 and (ref["refl"] & use).sum() > 300 and (ref["cos_t"] == 0).sum() > 300
    assert (got[:, 7] == np.float32(bp[4])).sum() > 500 and (got[:, 7] == np.float32(bp[5])).sum() > 300
    # wi.z == 0: weight 0; +-1e-4 are ordinary rows (compared above)
    assert (got[0, 3:7] == 0).all() and got[0, 7] == 1.0
    assert not exempt[1] and not exempt[2]
    # beyond the critical angle every sample reflects with F = 1; just within it u0 -> 1 transmits
    assert (got[3:22, 7] == 1.0).all() and (got[3:22, 6] == 1.0).all() and (got[3:22, 2] < 0).all()
    assert (got[22:40, 7] == np.float32(bp[5])).all() and (got[22:40, 2] > 0).all()
    # u0 = 0 reflects
    assert (got[40:60, 7] == 1.0).all() and (np.sign(got[40:60, 2]) == np.sign(W[40:60, 2])).all()
    # the ties: reflection at u0 == F, transmission at the next float
    for i in tie:
        assert (got[i, 7] == 1.0) == (i % 2 == 0), i
        assert abs(float(U0[i]) - ref["F"][i]) < 2.0 ** -23


def test_conductor_host_matches_float64(pkg, scenes):
    bp = scenes.smooth_conductor_params((0.9, 0.8, 0.7), eta=1.2, k=7.0)
    host = HostSmooth(pkg, bp)
    rng = np.random.default_rng(4100)
    W = sphere_wi(rng, NQ)
    W[0] = (0.6, 0.8, 0.0)
    W[1] = (0.6, 0.8, 1e-4)
    W[2] = (0.6, 0.8, -1e-4)
    W[3] = (0.0, 0.0, 1.0)
    got = host.sample_rows(W, rng.uniform(0, 1, NQ).astype(np.float32))
    ref = conductor_sample64(W, bp)
    e_wo, e_w, e_p = ulps(got[:, :3], ref["wo"]).max(), ulps(got[:, 3:6], ref["w"]).max(), ulps(got[:, 6], ref["pdf"]).max()
    print(f"smooth conductor host: worst ulp wo {e_wo:.3g}, weight {e_w:.3g}, pdf {e_p:.3g}; "
          f"{int(ref['void'].sum())} of {NQ} from behind")
    assert max(e_wo, e_w, e_p) <= 1.0 and (got[:, 7] == 1.0).all()
    assert ref["void"].sum() > 1500 and (~ref["void"]).sum() > 1500
    assert (got[0, 3:7] == 0).all() and (got[2, 3:7] == 0).all() and got[1, 6] == 1.0
    # other parameters, a dielectric-like k = 0 among them
    for eta, k in ((0.2, 3.9), (1.5, 0.0), (2.9, 3.1)):
        bp2 = scenes.smooth_conductor_params(eta=eta, k=k)
        h2 = HostSmooth(pkg, bp2)
        g2 = h2.sample_rows(W[:600], np.zeros(600, np.float32))
        assert ulps(g2[:, 3:6], conductor_sample64(W[:600], bp2)["w"]).max() <= 1.0


def _rotated(v, angle, rng):
    """v turned by `angle` about a random axis perpendicular to it (float64)."""
    v = np.asarray(v, np.float64)
    a = np.cross(v, rng.normal(size=3))
    a /= np.linalg.norm(a)
    return v * np.cos(angle) + np.cross(a, v) * np.sin(angle)


def test_eval_mode(pkg, scenes):
    """EDiscrete eval / pdf: at the sampled wo the lobe's weight * pdf (of the
    float64 restatement, within 1 float32 ulp) and the sample's pdf and eta; the same within DeltaEpsilon (a turn of 0.01
    rad: 1 - cos = 5e-5); 0 beyond it (0.1 rad: 5e-3 > 1e-3)."""
    rng = np.random.default_rng(77)
    bp, st = glass_params(scenes)
    cbp = scenes.smooth_conductor_params((0.9, 0.8, 0.7))
    n_r = n_t = n_c = 0
    for host, params in ((HostSmooth(pkg, bp, st), bp), (HostSmooth(pkg, cbp), cbp)):
        diel = params[0] == 5.0
        for wi in sphere_wi(rng, 400):
            if abs(wi[2]) < 0.05:
                continue
            u0 = np.float32(rng.uniform())
            wo, w, p, e = host.sample(wi, u0)
            f, pe, ee = host.eval(wi, wo)
            r64 = dielectric_sample64(wi[None], [u0], params, st) if diel else conductor_sample64(wi[None], params)
            if p == 0:
                assert not diel and wi[2] < 0 and (f == 0).all() and pe == 0
                continue
            assert pe == p and ee == e
            # (the float64 weight * pdf rounded once: the float32 pair's product is rounded three times)
            assert ulps(f, r64["w"][0] * r64["pdf"][0]).max() <= 1.0
            n_c += not diel
            n_r += diel and e == 1.0
            n_t += diel and e != 1.0
            near = _rotated(wo, 0.01, rng)
            far = _rotated(wo, 0.1, rng)
            if near[2] * wo[2] > 0 and far[2] * wo[2] > 0:
                f2, p2, e2 = host.eval(wi, near)
                assert (f2 == f).all() and p2 == p and e2 == e
                f3, p3, _ = host.eval(wi, far)
                assert (f3 == 0).all() and p3 == 0
        # the other lobe's side without its direction: 0
        f, p, _ = host.eval(np.float32([0.6, 0.0, 0.8]), np.float32([0.6, 0.0, -0.8]))
        assert (f == 0).all() and p == 0
    assert n_r > 20 and n_t > 200 and n_c > 100
    # wi.z == 0 evaluates to 0
    f, p, _ = HostSmooth(pkg, bp, st).eval(np.float32([0.6, 0.8, 0.0]), np.float32([-0.6, -0.8, 0.0]))
    assert (f == 0).all() and p == 0


def test_entry_point_arguments(pkg, scenes):
    """The calls dispatch on params[0] and refuse another kind's row."""
    bp4, st = scenes.dielectric_params()
    with pytest.raises(pkg.SDMMError, match="kind-5 or kind-6"):
        pkg.bsdf_smooth_host(bp4, st, [0.0, 0.0, 1.0], u=[0.5, 0.5])
    bp, st = glass_params(scenes)
    wo, w, p, e = pkg.bsdf_smooth_host(bp, st, [0.0, 0.0, 1.0], u=[0.0, 0.5])
    assert (wo == [0.0, 0.0, 1.0]).all() and (w == bp[1:4]).all() and e == 1.0
    F = ((ETA - 1) / (ETA + 1)) ** 2
    assert abs(p - F) < 1e-6
    wo, w, p, e = pkg.bsdf_smooth_host(bp, st, [0.0, 0.0, 1.0], u=[0.9, 0.5])
    assert (wo == [0.0, 0.0, -1.0]).all() and e == bp[4] and abs(p - (1 - F)) < 1e-6
    np.testing.assert_allclose(w, st / np.float64(bp[4]) ** 2, rtol=2e-7)
    wo, w, p, e = pkg.bsdf_smooth_host(scenes.smooth_conductor_params(), None, [0.0, 0.6, 0.8], u=[0.3, 0.3])
    assert (wo == np.float32([0.0, -0.6, 0.8])).all() and p == 1.0 and e == 1.0 and (w > 0.8).all() and (w < 1).all()
    with pytest.raises(pkg.SDMMError):
        pkg.bsdf_smooth_host(bp, st, [0.0, 0.0, 1.0], u=[0.5, 0.5, 0.5])


def test_scene_rejects_invalid_smooth_params(pkg, scenes):
    names = list(scenes._BSDFS)
    g, m = names.index("TallBox"), names.index("BackWall")

    def scene():
        return scenes.cornell_box(32, 18, glass=("TallBox",), mirror=("BackWall",), dielectric_lift=0.02)
    desc = scene()
    assert desc["bsdf_params"][8 * g] == 5.0 and desc["bsdf_params"][8 * m] == 6.0 and "learned_models_nd" not in desc
    bad = [(g, 4, 1.0), (g, 4, 0.0), (g, 4, -1.5), (g, 4, np.nan), (g, 4, np.inf), (g, 5, 0.0), (g, 5, -0.6),
           (g, 5, np.inf), (g, 1, -0.1), (g, 2, np.nan), (g, 3, np.inf),
           (m, 4, 0.0), (m, 4, -1.2), (m, 4, np.nan), (m, 4, np.inf), (m, 5, -1.0), (m, 5, np.inf), (m, 5, np.nan),
           (m, 1, -0.1), (m, 3, np.nan), (m, 0, 7.0)]
    for b, slot, value in bad:
        desc = scene()
        desc["bsdf_params"][8 * b + slot] = value
        with pytest.raises(pkg.SDMMError, match="invalid bsdf_params"):
            pkg.Scene(desc)
    for value in (-0.5, np.nan, np.inf):                    # the dielectric's transmittance row
        desc = scene()
        desc["reflectance"][3 * g + 1] = value
        with pytest.raises(pkg.SDMMError, match="invalid bsdf_params.*transmittance"):
            pkg.Scene(desc)
    with pytest.raises(ValueError):
        scenes.smooth_dielectric_params(int_ior=1.5, ext_ior=1.5)
    with pytest.raises(ValueError):
        scenes.cornell_box(32, 18, glass=("TallBox",), dielectric=("TallBox",))


def test_scene_helpers(scenes):
    """The selectors' defaults leave every scene as it was; smooth=True swaps
    the torus scene's case and two arcs of the ring."""
    a, b = scenes.torus_scene(64, 36, nu=32, nv=16), scenes.torus_scene(64, 36, nu=32, nv=16, smooth=False)
    assert a.keys() == b.keys() and "Metal" not in a
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes()
    s = scenes.torus_scene(64, 36, nu=32, nv=16, smooth=True)
    bp = s["bsdf_params"].reshape(-1, 8)
    assert bp[3, 0] == 5.0 and bp[3, 4] == np.float32(1.5) and bp[5, 0] == 6.0 and "learned_models_nd" not in s
    metal = s["tri_bsdf"] == 5
    assert metal.sum() == len(metal) // 4 and (s["tri_bsdf"][~metal] == 2).all()
    assert (s["quads"] == a["quads"]).all() and (s["triangles"] == a["triangles"]).all()
    c0 = scenes.cornell_box(32, 18)
    c1 = scenes.cornell_box(32, 18, glass=(), mirror=())
    assert c0.keys() == c1.keys() and all(np.array_equal(c0[k], c1[k]) for k in c0 if isinstance(c0[k], np.ndarray))
