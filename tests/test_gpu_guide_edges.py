"""The guided bounce on CONSTRUCTED mixtures: ties, invalid conditionals with
real mass, the underflow band, non-finite queries, edge uniforms and edge
directions -- the branches of guide.hip that an EM-fitted mixture and random
queries never take ("Guide: constructed edge families").

A case is K means (position, unit direction) and K 5x5 tangent covariances
built in numpy, loaded with set_params and read back into an oracle.Mixture
(the _em_model pattern of test_gpu_parity.py: both sides hold the same derived
floats).  The CPU-only test builds the same mixtures with the oracle's own
set_component + configure and asserts that every family still reaches the
branch it was built for.

Families (numbers: the oracle's own, nq = 1024):
  clones     K copies of one component: every query a K-way tie, comp == slot;
  pairs      components k and k + K/2 identical: the upper twin is the answer
             for about half the queries;
  sparse     pairs with three of every four weights exactly 0;
  steep      rho = 0.99, sd in [2, 3]: the heaviest component's conditional is
             invalid (tangent length >= pi) for 10..50 % of the queries;
  broad      every conditional valid; u1 = 1 - 2^-24 samples direction 0;
  underflow  q in 150..190 around NORM3 exp(-q/2) = FLT_MIN (q = 169.16);
  nonfinite  NaN / +inf / -inf query coordinates beside ordinary queries.

Tolerances (the project's existing ones): index and h exact; d 1e-5 abs; pdf
1e-4 rel + 1e-7 abs; product d 1e-6 abs, product pdf 1e-5 rel + 1e-8 abs.
Two exclusions, decided from the oracle's output alone, apply to d and pdf
(never to comp):
  * the oracle's own direction is neither 0 nor unit (|norm - 1| > 1e-4: at
    u0 = 0 with an invalid conditional in slot 0 the reference samples around
    a zero mean direction) -- at most 5 % of a case;
  * the oracle's pdf moves by more than 3e-5 rel + 1e-7 abs under one of four
    renormalised 3e-7 perturbations of d -- at most 1 % of a case.
"""
import numpy as np
import pytest

KS = (16, 72, 128, 512)
# two and four slots per lane of the 16-lane group fallback (K in (16, 32] and
# (32, 64], no multiple of 16): K = 16, 72 and 128 run its 1- and 8-slot forms.
# Run with clones (the tie order) and steep (invalid conditionals), whose
# conditional sigma (<= 0.42) keeps the u1 = 1 - 2^-24 sample (radius 5.77
# sigma) away from pi.  Not pairs: its sigma ranges over pi / 5.77 = 0.544,
# and at K = 40 one twin pair lands within 1e-3 of it, so that every such
# sample sits on the antipode of its own mean, where the reference's pdf
# jumps (sin < 1e-3 -> J = 1) under a 2.5e-7 move of d: 13 such rows on the
# oracle alone, of which the four-probe exclusion below sees 6.
GROUP_KS = (24, 40)
NQ = 1024
EDGE = np.float32(1.0 - 2.0 ** -24)          # the largest float below 1
NORM3 = float(np.float32(np.float32(0.3989422804014327) ** 3))

D_ATOL = 1e-5
PDF_RTOL, PDF_ATOL = 1e-4, 1e-7
PROD_D_ATOL = 1e-6
PROD_PDF_RTOL, PROD_PDF_ATOL = 1e-5, 1e-8
NONUNIT_MAX = 0.05
ILLCOND_MAX = 0.01


# ---------------------------------------------------------------------------
# builders (numpy, fp64)

def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def cov5(sp, sd, rho):
    """diag(sp^2 x3, sd^2 x2) with entries (0,3), (3,0), (1,4), (4,1) = rho sp sd."""
    c = np.diag([sp * sp, sp * sp, sp * sp, sd * sd, sd * sd]).astype(np.float64)
    c[0, 3] = c[3, 0] = c[1, 4] = c[4, 1] = rho * sp * sd
    return c


def _random_components(K, n, sp, sd, rho):
    """n components drawn with default_rng(100 + K): sp, sd, rho uniform in
    the given (lo, hi), then position uniform in the unit box, direction a
    normalised normal, weights rand + 0.1.  (The order is a choice: with the
    covariance scalars drawn last, steep at K = 16 puts an invalid conditional
    in slot 0 of 60 % of the u0 = 0 queries and 6.0 % of the oracle's
    directions are non-unit, over the 5 % cap that
    test_families_hit_their_branches holds on the oracle alone; this order
    gives 3.3 %.)"""
    rng = np.random.default_rng(100 + K)
    sps, sds, rhos = (rng.uniform(lo, hi, size=n) for lo, hi in (sp, sd, rho))
    pos = rng.uniform(0.0, 1.0, size=(n, 3))
    d = unit(rng.normal(size=(n, 3)))
    w = rng.random(n) + 0.1
    cov = np.stack([cov5(a, b, r) for a, b, r in zip(sps, sds, rhos)])
    return w / w.sum(), np.concatenate([pos, d], 1), cov


CLONE_MEAN = np.concatenate([[0.3, 0.4, 0.5], unit([0.2, 0.3, 0.9])])


def family(name, K, nq=NQ):
    """(weights (K,), means (K, 6), covs (K, 5, 5), queries c (nq, 3) float32)."""
    qr = np.random.default_rng(200 + K)
    box = lambda: qr.uniform(0.0, 1.0, size=(nq, 3)).astype(np.float32)
    if name == "clones":
        w = np.full(K, 1.0 / K)
        mean = np.tile(CLONE_MEAN, (K, 1))
        cov = np.tile(cov5(0.2, 0.4, 0.3), (K, 1, 1))
        c = (CLONE_MEAN[:3] + 0.2 * qr.normal(size=(nq, 3))).astype(np.float32)
    elif name in ("pairs", "sparse"):
        w, mean, cov = _random_components(K, K // 2, (0.15, 0.35), (0.3, 0.6), (0.0, 0.5))
        w, mean, cov = np.concatenate([w, w]) / 2, np.concatenate([mean, mean]), np.concatenate([cov, cov])
        if name == "sparse":
            w[np.arange(K) % 4 != 0] = 0.0      # K/2 is a multiple of 4: both twins survive
            w /= w.sum()
        c = box()
    elif name == "steep":
        w, mean, cov = _random_components(K, K, (0.1, 0.2), (2.0, 3.0), (0.99, 0.99))
        c = box()
    elif name == "broad":
        w, mean, cov = _random_components(K, K, (0.1, 0.2), (0.6, 0.8), (0.0, 0.0))
        c = box()
    elif name == "underflow":
        w = np.full(K, 1.0 / K)
        mean = np.tile(np.concatenate([[0.5, 0.5, 0.5], CLONE_MEAN[3:]]), (K, 1))
        cov = np.tile(cov5(0.01, 0.4, 0.0), (K, 1, 1))
        q = UNDERFLOW_Q
        c = np.full((len(q), 3), 0.5, np.float32)
        c[:, 0] = (0.5 + 0.01 * np.sqrt(q)).astype(np.float32)
    elif name == "nonfinite":
        rng = np.random.default_rng(100 + K)
        pos = rng.uniform(0.0, 1.0, size=(K, 3))
        d = unit(rng.normal(size=(K, 3)))
        w = rng.random(K) + 0.1
        w /= w.sum()
        mean = np.concatenate([pos, d], 1)
        scale = np.array([0.2, 0.2, 0.2, 0.5, 0.5])
        cov = np.empty((K, 5, 5))
        for k in range(K):
            a = rng.normal(size=(5, 5))
            m = a @ a.T + 5.0 * np.eye(5)        # full SPD, correlations ~0.3
            s = np.sqrt(np.diag(m))
            cov[k] = m / np.outer(s, s) * np.outer(scale, scale)
        cov[0::3] = cov5(0.2, 0.5, 0.2)          # margL off-diagonals exactly 0: inf * 0 = NaN
        c = box()
        i = np.arange(nq) % 4
        c[i == 0, 0] = np.nan
        c[i == 1, 1] = np.inf
        c[i == 2, 2] = -np.inf
    else:
        raise KeyError(name)
    return w, mean, cov, c


UNDERFLOW_Q = 150.0 + 0.1 * np.arange(401)


def u_planes(nq, seed):
    """Plain uniforms (nq, 3); in every run of seven queries one plane carries
    an edge value in turn: u1 = 1 - 2^-24, u1 = 0, u0 = 0, u0 = 1, u2 = 0,
    u2 = 1 - 2^-24 (the seventh query is plain)."""
    rng = np.random.default_rng(seed)
    u = np.minimum(rng.random((nq, 3)).astype(np.float32), EDGE)
    i = np.arange(nq) % 7
    u[i == 0, 1] = EDGE
    u[i == 1, 1] = 0.0
    u[i == 2, 0] = 0.0
    u[i == 3, 0] = 1.0
    u[i == 4, 2] = 0.0
    u[i == 5, 2] = EDGE
    return u


def clone_ladder(u, L):
    """u0 = j / L and both float neighbours, j = 0..L (L: the oracle's kept
    length per query), on the rows whose u0 is not an edge value; all 3 (L + 1)
    values when they fit the batch, an even spread of them otherwise."""
    nq = len(u)
    i = np.arange(nq)
    n = 3 * (int(L.max()) + 1)
    t = i % n if n <= nq else (i * n) // nq
    j = np.minimum(t // 3, L)
    x = (j / L).astype(np.float32)
    val = np.stack([np.nextafter(x, np.float32(-1)), x, np.nextafter(x, np.float32(2))])[t % 3, i]
    rows = ~np.isin(i % 7, (2, 3))
    u[rows, 0] = np.clip(val, 0.0, 1.0)[rows]
    return u


# ---------------------------------------------------------------------------
# the oracle side

def oracle_mixture(oracle, w, mean, cov):
    """The family on the oracle alone: set_component + configure."""
    K = len(w)
    m = oracle.Mixture(K)
    for k in range(K):
        assert m.set_component(k, mean[k], cov[k].reshape(25), 1) == 1
    m.weights[:] = w.astype(np.float32)
    assert m.configure() == 1
    return m


def _perturbed(d):
    """Four renormalised 3e-7 perturbations of the directions d (n, 3): +-3e-7
    along two tangents, scaled back to the length of d."""
    d64 = d.astype(np.float64)
    n = np.linalg.norm(d64, axis=1, keepdims=True)
    e = d64 / np.where(n > 0, n, 1.0)
    a = np.where(np.abs(e[:, :1]) < 0.9, [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]])
    t1 = np.cross(e, a)
    t1 /= np.maximum(np.linalg.norm(t1, axis=1, keepdims=True), 1e-30)
    t2 = np.cross(e, t1)
    for t in (t1, -t1, t2, -t2):
        p = d64 + 3e-7 * n * t
        p *= n / np.maximum(np.linalg.norm(p, axis=1, keepdims=True), 1e-30)
        yield p.astype(np.float32)


def ill_conditioned(pdf_at, d, p0):
    """Rows whose oracle pdf moves by more than 3e-5 rel + 1e-7 abs under one
    of the four perturbations (pdf_at(d') -> the oracle's pdf at d'); zero and
    non-finite directions are not perturbed."""
    ok = np.isfinite(d).all(1) & (np.abs(d).sum(1) > 0)
    bad = np.zeros(len(d), bool)
    for dp in _perturbed(np.where(ok[:, None], d, np.float32([0, 0, 1]))):
        with np.errstate(invalid="ignore"):
            bad |= ok & (np.abs(pdf_at(dp).astype(np.float64) - p0) > 3e-5 * np.abs(p0) + 1e-7)
    return bad


def non_unit(d):
    """The oracle's direction is neither 0 nor unit (NaN directions: neither)."""
    with np.errstate(invalid="ignore"):
        n = np.linalg.norm(d.astype(np.float64), axis=1)
        return (n != 0) & (np.abs(n - 1.0) > 1e-4)


def reference(oracle, om, name, c):
    """Everything a case's tests share, computed once: u planes, the oracle's
    guided bounce, its exclusion masks."""
    nq = len(c)
    u = u_planes(nq, 300 + om.K)
    if name == "clones":
        u1 = u.copy()
        u1[:, 0] = 1.0                            # the tie walk: the last kept slot
        L = oracle.guide_batch(om, c, u1)[3] + 1
        assert (L > 0).all()
        u = clone_ladder(u, L)
    dr, pr, cr, sr = oracle.guide_batch(om, c, u)
    nonunit = non_unit(dr)
    ill = ill_conditioned(lambda dp: oracle.pdf_batch(om, c, dp), dr, pr.astype(np.float64)) & ~nonunit
    return {"c": c, "u": u, "d": dr, "pdf": pr, "comp": cr, "slot": sr, "nonunit": nonunit, "ill": ill}


def check_exclusions(ref, plog=None, tag=""):
    fu, fi = float(ref["nonunit"].mean()), float(ref["ill"].mean())
    if plog is not None:
        plog(f"{tag}_excluded_nonunit_share", fu, NONUNIT_MAX)
        plog(f"{tag}_excluded_illcond_share", fi, ILLCOND_MAX)
    assert fu <= NONUNIT_MAX, f"{tag}: {fu:.3f} of the oracle's directions are neither 0 nor unit"
    assert fi <= ILLCOND_MAX, f"{tag}: {fi:.3f} of the oracle's pdfs are ill-conditioned"


def marginal_f64(om, c):
    """fp64 marginal weights (nq, K), their Mahalanobis q, and the tangent
    length of every conditional mean, from the oracle's mean, cov, muPremult
    and weights."""
    K = om.K
    mean = om.mean.astype(np.float64)[:, :3]
    cov = om.cov.astype(np.float64).reshape(K, 5, 5)[:, :3, :3]
    diff = c.astype(np.float64)[:, None, :] - mean[None]
    q = np.einsum("nki,kij,nkj->nk", diff, np.linalg.inv(cov), diff)
    w = om.weights.astype(np.float64) * NORM3 * np.exp(-0.5 * q) / np.sqrt(np.linalg.det(cov))
    t = np.einsum("kij,nkj->nki", om.muPremult.astype(np.float64).reshape(K, 2, 3), diff)
    return w, q, np.linalg.norm(t, axis=-1)


# ---------------------------------------------------------------------------
# CPU: the families reach their branches (oracle only)

@pytest.mark.parametrize("name", ["clones", "pairs", "sparse", "steep", "broad"])
def test_families_hit_their_branches(oracle, name):
    """What keeps a later edit of a builder from quietly emptying a case: the
    facts each family was built for, recomputed in fp64 numpy from the
    oracle's parameters or read off the oracle's answers, with margin; and
    the two exclusion caps on the oracle alone."""
    for K in KS + (GROUP_KS if name in ("clones", "steep") else ()):
        w, mean, cov, c = family(name, K)
        om = oracle_mixture(oracle, w, mean, cov)
        ref = reference(oracle, om, name, c)
        check_exclusions(ref, tag=f"{name}_K{K}")
        wq, q, tlen = marginal_f64(om, c)
        # no query of these families is a zero-mass one: at capacity 0 every
        # query reaches the fallback list
        assert (q.min(1) < 150.0).all()
        comp, slot = ref["comp"], ref["slot"]
        if name == "clones":
            np.testing.assert_array_equal(comp, slot)          # a K-way tie in index order
            assert slot.max() == {16: 15, 24: 23, 40: 39, 72: 71, 128: 126, 512: 506}[K]
            assert (tlen < np.pi).all()
        if name in ("pairs", "sparse"):
            upper = float((comp >= K // 2).mean())
            assert 0.3 <= upper <= 0.7, upper
            assert (comp >= 0).all()
        if name == "sparse":
            assert (w[comp] > 0).all() and int((w == 0).sum()) == 3 * K // 4
        if name == "steep":
            heavy = wq.argmax(1)
            share = float((tlen[np.arange(len(c)), heavy] >= np.pi).mean())
            assert share >= 0.05, (K, share)
            if K == 16:
                assert ((comp == -1) & (wq.sum(1) > 1e-30)).mean() > 0
        else:
            assert not ref["nonunit"].any()                    # occurs only in steep
        if name == "broad":
            assert (tlen < np.pi).all()                        # every conditional valid
            zero = (np.abs(ref["d"]).sum(1) == 0) & (comp >= 0)
            assert zero.mean() >= 0.05, zero.mean()
            assert zero[np.arange(len(c)) % 7 == 0].all()      # u1 = 1 - 2^-24: radius 5.77


def test_underflow_family_hits_the_band(oracle):
    for K in (16, 128):
        w, mean, cov, c = family("underflow", K)
        om = oracle_mixture(oracle, w, mean, cov)
        np.testing.assert_allclose(om.margDetInv, 1e6, rtol=1e-5)
        comp = reference(oracle, om, "underflow", c)["comp"]
        first = int(np.argmax(comp == -1))
        assert 169.1 <= UNDERFLOW_Q[first] <= 169.3, UNDERFLOW_Q[first]
        assert (comp[first:] == -1).all() and (comp[:first] >= 0).all()
        assert int((comp == -1).sum()) == 209


def test_nonfinite_family_answers(oracle):
    for K in (16, 128, 512):
        w, mean, cov, c = family("nonfinite", K)
        om = oracle_mixture(oracle, w, mean, cov)
        ref = reference(oracle, om, "nonfinite", c)
        i = np.arange(len(c)) % 4
        for rows in (i == 0, i == 1):                          # NaN x, +inf y
            assert (ref["comp"][rows] == 0).all()
            assert np.isnan(ref["d"][rows]).all() and np.isnan(ref["pdf"][rows]).all()
        assert (ref["comp"][i == 2] == -1).all() and (ref["pdf"][i == 2] == 0).all()   # -inf z
        plain = i == 3
        assert np.isfinite(ref["d"][plain]).all() and np.isfinite(ref["pdf"][plain]).all()
        alone = oracle.guide_batch(om, c[plain], ref["u"][plain])
        np.testing.assert_array_equal(alone[2], ref["comp"][plain])
        np.testing.assert_array_equal(alone[1], ref["pdf"][plain])
        check_exclusions(ref, tag=f"nonfinite_K{K}")


# ---------------------------------------------------------------------------
# GPU

_CASES = {}


def device_case(pkg, oracle, name, K):
    """(device mixture, oracle mixture of its read-back parameters, shared
    reference) of a family, built once per (family, K)."""
    key = (name, K)
    if key not in _CASES:
        w, mean, cov, c = family(name, K)
        mix = pkg.SDMM(K)
        mix.set_params(w, mean, cov.reshape(K, 25))
        p = mix.get_params()
        om = oracle.Mixture(K)
        om.copy_params_from(p)
        om.valid[:] = p["valid"]
        assert (p["valid"] == 1).all()
        _CASES[key] = (mix, om, reference(oracle, om, name, c), {})
    return _CASES[key]


def planes(gpu, a):
    """(n, 3) host array -> three device planes."""
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a[:, i])).to(gpu) for i in range(a.shape[1])]


def run_guide(mix, gpu, c, u):
    import torch
    d, pdf, comp = mix.guide(planes(gpu, c), planes(gpu, u))
    torch.cuda.synchronize()
    return np.stack([t.cpu().numpy() for t in d], 1), pdf.cpu().numpy(), comp.cpu().numpy()


def compare(plog, tag, got, ref, rows=None, d_atol=D_ATOL, pdf_rtol=PDF_RTOL, pdf_atol=PDF_ATOL):
    """comp bit-equal on every row; d and pdf within tolerance outside the two
    exclusions; NaN positions equal.  Every realised maximum is logged first."""
    dg, pg, cg = got
    sel = np.ones(len(cg), bool) if rows is None else rows
    dr, pr, cr = ref["d"], ref["pdf"], ref["comp"]
    keep_d = sel & ~ref["nonunit"]
    keep_p = keep_d & ~ref["ill"]
    with np.errstate(invalid="ignore"):
        derr = np.abs(dg[keep_d].astype(np.float64) - dr[keep_d])
        perr = np.abs(pg[keep_p].astype(np.float64) - pr[keep_p]) / (pdf_atol + pdf_rtol * np.abs(pr[keep_p]))
    plog(f"{tag}_index_mismatches", int((cg[sel] != cr[sel]).sum()), 0)
    plog(f"{tag}_dir_abs_err", np.nanmax(derr, initial=0.0), d_atol)
    plog(f"{tag}_pdf_err_over_tol", np.nanmax(perr, initial=0.0), 1.0)
    np.testing.assert_array_equal(cg[sel], cr[sel])
    np.testing.assert_array_equal(np.isnan(dg[sel]), np.isnan(dr[sel]))
    np.testing.assert_array_equal(np.isnan(pg[sel]), np.isnan(pr[sel]))
    np.testing.assert_allclose(dg[keep_d], dr[keep_d], rtol=0, atol=d_atol)
    np.testing.assert_allclose(pg[keep_p], pr[keep_p], rtol=pdf_rtol, atol=pdf_atol)


GUIDE_CASES = [(n, K, cap) for n in ("clones", "pairs", "sparse", "steep", "broad") for K in KS for cap in (40, 4, 0)]
# every guide_cand_kernel<LCAP> instance (16, 24, 40, 64) at K = 128
GUIDE_CASES += [(n, 128, cap) for n in ("clones", "steep") for cap in (16, 24, 64)]
GUIDE_CASES += [(n, K, cap) for n in ("clones", "steep") for K in GROUP_KS for cap in (4, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,K,cap", GUIDE_CASES)
def test_guide_constructed(pkg, oracle, gpu, plog, name, K, cap):
    """Families 1-5 through the candidate list (capacity 40: LCAP 16 at K = 16,
    40 above), a list that mostly overflows (4) and the full-K path alone (0:
    the 16-lane groups up to K = 128, one wave per query at K = 512)."""
    mix, om, ref, _ = device_case(pkg, oracle, name, K)
    tag = f"{name}_K{K}_cap{cap}"
    check_exclusions(ref, plog, tag)
    mix.set_guide_capacity(cap)
    got = run_guide(mix, gpu, ref["c"], ref["u"])
    fb = mix.guide_fallback_count()
    plog(f"{tag}_fallbacks", fb, NQ)
    compare(plog, tag, got, ref)
    if cap == 0:
        assert fb == NQ                       # no zero-mass query in these families
    elif name == "clones" and (K >= 72 or cap < K):
        assert fb == NQ                       # the kept prefix (K, 127, 507) exceeds every list
    elif name == "clones" and K == 16 and cap == 40:
        assert fb == 0
    # short batches (one lane, a wave minus / plus one) on the first rows: the
    # same bits as the rows of the full batch
    for n in (1, 63, 65):
        dn, pn, cn = run_guide(mix, gpu, ref["c"][:n], ref["u"][:n])
        np.testing.assert_array_equal(cn, ref["comp"][:n])
        np.testing.assert_array_equal(cn, got[2][:n])
        np.testing.assert_array_equal(dn, got[0][:n])
        np.testing.assert_array_equal(pn, got[1][:n])


def pdf_directions(oracle, om, ref):
    """Directions of test_pdf_constructed, in turn: a random unit vector, the
    oracle's own sampled direction, the zero vector, twice a unit vector, the
    oracle's sampled direction at u1 = 0 (the conditional mean itself: the
    sin < 1e-3 and cos >= 1 clamp branches) and that mean's exact antipode
    (kind 5: not compared -- the reference formula jumps there from 0 to the
    mode's density)."""
    c, u = ref["c"], ref["u"]
    nq = len(c)
    rng = np.random.default_rng(400 + om.K)
    d = unit(rng.normal(size=(nq, 3))).astype(np.float32)
    kind = np.arange(nq) % 6
    u0 = u.copy()
    u0[:, 1] = 0.0
    mean_dir = oracle.guide_batch(om, c, u0)[0]
    d[kind == 1] = ref["d"][kind == 1]
    d[kind == 2] = 0.0
    d[kind == 3] *= 2.0
    d[kind == 4] = mean_dir[kind == 4]
    d[kind == 5] = -mean_dir[kind == 5]
    return d, kind


@pytest.mark.gpu
@pytest.mark.parametrize("name,K,cap", [(n, K, cap) for n in ("pairs", "steep", "broad") for K in KS
                                        for cap in (40, 0)])
def test_pdf_constructed(pkg, oracle, gpu, plog, name, K, cap):
    import torch
    mix, om, ref, memo = device_case(pkg, oracle, name, K)
    tag = f"pdf_{name}_K{K}_cap{cap}"
    if "pdf" not in memo:
        d, kind = pdf_directions(oracle, om, ref)
        pr = oracle.pdf_batch(om, ref["c"], d)
        ill = ill_conditioned(lambda dp: oracle.pdf_batch(om, ref["c"], dp), d, pr.astype(np.float64))
        memo["pdf"] = (d, kind, pr, ill)
    d, kind, pr, ill = memo["pdf"]
    mix.set_guide_capacity(cap)
    got = mix.pdf(planes(gpu, ref["c"]), planes(gpu, d)).cpu().numpy()
    torch.cuda.synchronize()
    cmp_rows = kind != 5
    # the clamp branches are taken: the zero vector gives exactly 0, and the
    # oracle's pdf at a conditional mean is that of a mode
    assert (pr[kind == 2] == 0).all() and (got[kind == 2] == 0).all()
    assert np.isfinite(got).all() and (got >= 0).all()
    share = float((ill & cmp_rows).mean())
    plog(f"{tag}_excluded_illcond_share", share, ILLCOND_MAX)
    assert share <= ILLCOND_MAX
    keep = cmp_rows & ~ill
    err = np.abs(got[keep].astype(np.float64) - pr[keep]) / (PDF_ATOL + PDF_RTOL * np.abs(pr[keep]))
    for k, label in enumerate(("random", "sampled", "zero", "twice_unit", "cond_mean")):
        plog(f"{tag}_{label}_err_over_tol", err[kind[keep] == k].max(initial=0.0), 1.0)
    np.testing.assert_allclose(got[keep], pr[keep], rtol=PDF_RTOL, atol=PDF_ATOL)


@pytest.mark.gpu
@pytest.mark.parametrize("K,cap", [(K, cap) for K in (16, 128) for cap in (40, 0)])
def test_underflow_band(pkg, oracle, gpu, plog, K, cap):
    """kMarginalZeroQ = 170 skips the double exp; the reference's weight already
    flushes at q = 169.16.  In between the device forms (float)(double) of a
    value below FLT_MIN and must reach the same exact 0 (margDetInv = 1e6: a
    weight that is not flushed is a live component).  comp bit for bit on all
    401 queries; pdf bit for bit on every query of the band and beyond it
    (q > 169.16: the reference's answer is comp -1, pdf 0).  Below the band the
    query is live and its pdf is the float-transcendental one of every other
    guide test (1e-4 rel + 1e-7): measured 71 of the 192 live rows at K = 16
    (35 at K = 128) differ from the oracle in the last bits, by at most
    1.1e-5 relative -- logged, not a flush question."""
    mix, om, ref, _ = device_case(pkg, oracle, "underflow", K)
    tag = f"underflow_K{K}_cap{cap}"
    check_exclusions(ref, plog, tag)
    mix.set_guide_capacity(cap)
    got = run_guide(mix, gpu, ref["c"], ref["u"])
    dg, pg, cg = got
    dead = ref["comp"] == -1
    assert int(dead.sum()) == 209
    band = UNDERFLOW_Q > 169.16
    np.testing.assert_array_equal(band, dead)         # the reference flushes exactly there
    in_band = band & (UNDERFLOW_Q <= 170.0)           # ... of which the device still runs the exp for these
    assert int(in_band.sum()) == 9
    bits = pg.view(np.uint32) != ref["pdf"].view(np.uint32)
    plog(f"{tag}_band_pdf_bit_mismatches", int(bits[band].sum()), 0, band_rows=int(in_band.sum()))
    plog(f"{tag}_live_pdf_bit_mismatches", int(bits[~band].sum()), int((~band).sum()))
    compare(plog, tag, got, ref)                      # comp exact on every row; live rows within tolerance
    np.testing.assert_array_equal(pg.view(np.uint32)[band], ref["pdf"].view(np.uint32)[band])
    assert (dg[band] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("K,cap", [(K, cap) for K in (16, 128, 512) for cap in (40, 0)])
def test_nonfinite_queries(pkg, oracle, gpu, plog, K, cap):
    """NaN x, +inf y, -inf z and an ordinary query in every four.  The oracle's
    rule is the one guide.hip's header states (lastIdx = K if never reached):
    NaN or +inf y -> comp 0 with NaN direction and pdf; -inf z -> comp -1,
    pdf 0.  K <= 128: candidate kernel -> 16-lane group (sees the NaN) -> the
    one-wave scan; K = 512: the one-wave scan directly."""
    mix, om, ref, _ = device_case(pkg, oracle, "nonfinite", K)
    tag = f"nonfinite_K{K}_cap{cap}"
    check_exclusions(ref, plog, tag)
    mix.set_guide_capacity(cap)
    got = run_guide(mix, gpu, ref["c"], ref["u"])
    compare(plog, tag, got, ref)
    plain = np.arange(NQ) % 4 == 3
    alone = run_guide(mix, gpu, ref["c"][plain], ref["u"][plain])
    for a, b in zip(alone, got):
        np.testing.assert_array_equal(a, b[plain])


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [64, 40, 0])
def test_wavefront_constructed(pkg, oracle, gpu, plog, cap):
    """The tree kernels (register key lists build_candidates_key<40> / <64>,
    the TREE group fallback, the tree one-wave fallback) on the constructed
    families: one split_to_depth(1) tree whose leaves hold clones / steep /
    pairs at K = 16 and 128, steep at K = 72, and one leaf without a mixture.
    Per leaf bit-equal to that leaf's own guide / pdf; comp equal to the oracle."""
    import torch
    t = pkg.STree(np.float32([0, 0, 0]), np.float32([1, 1, 1]))
    t.split_to_depth(1)
    nq = 4096
    rng = np.random.default_rng(77)
    c = rng.uniform(0.0, 1.0, size=(nq, 3)).astype(np.float32)
    u = u_planes(nq, 78)
    dd = unit(rng.normal(size=(nq, 3))).astype(np.float32)
    ct, ut, dt = planes(gpu, c), planes(gpu, u), planes(gpu, dd)
    node = t.find(ct).cpu().numpy()
    leaves = np.unique(node)
    assert len(leaves) == 8 and leaves.min() >= 0
    layout = [("clones", 16), ("steep", 128), ("pairs", 16), None, ("clones", 128), ("steep", 16), ("pairs", 128),
              ("steep", 72)]
    mixes = [None] * t.num_nodes
    oms = {}
    for v, fam in zip(leaves, layout):
        if fam is not None:
            mixes[v], oms[v] = device_case(pkg, oracle, *fam)[:2]
            mixes[v].set_guide_capacity(cap)
    wnode = torch.empty(nq, dtype=torch.int32, device=gpu)
    dw, pw, cw = t.guide(mixes, ct, ut, node_out=wnode)
    pdw = t.pdf(mixes, ct, dt)
    torch.cuda.synchronize()
    dw = np.stack([x.cpu().numpy() for x in dw], 1)
    pw, cw, pdw = pw.cpu().numpy(), cw.cpu().numpy(), pdw.cpu().numpy()
    np.testing.assert_array_equal(wnode.cpu().numpy(), node)
    aabb, child, _ = t.nodes()
    np.testing.assert_array_equal(node, oracle.stree_find(aabb, child, c))
    served = 0
    for v, fam in zip(leaves, layout):
        sel = np.nonzero(node == v)[0]
        assert len(sel) > 300
        if fam is None:                              # no mixture: BSDF only
            assert (cw[sel] == -1).all() and (pw[sel] == 0).all() and (pdw[sel] == 0).all()
            assert (dw[sel] == 0).all()
            continue
        idx = torch.from_numpy(sel).to(gpu)
        dl, pl, cl = mixes[v].guide([x[idx] for x in ct], [x[idx] for x in ut])
        pdl = mixes[v].pdf([x[idx] for x in ct], [x[idx] for x in dt])
        torch.cuda.synchronize()
        np.testing.assert_array_equal(cw[sel], cl.cpu().numpy())
        np.testing.assert_array_equal(pw[sel], pl.cpu().numpy())
        np.testing.assert_array_equal(dw[sel], np.stack([x.cpu().numpy() for x in dl], 1))
        np.testing.assert_array_equal(pdw[sel], pdl.cpu().numpy())
        om = oms[v]
        dr, pr, cr, _ = oracle.guide_batch(om, c[sel], u[sel])
        nonunit = non_unit(dr)
        ref = {"d": dr, "pdf": pr, "comp": cr, "nonunit": nonunit,
               "ill": ill_conditioned(lambda dp: oracle.pdf_batch(om, c[sel], dp), dr, pr.astype(np.float64)) & ~nonunit}
        tag = f"wavefront_cap{cap}_{fam[0]}_K{fam[1]}"
        check_exclusions(ref, plog, tag)
        compare(plog, tag, (dw[sel], pw[sel], cw[sel]), ref)
        pdr = oracle.pdf_batch(om, c[sel], dd[sel])
        ill = ill_conditioned(lambda dp: oracle.pdf_batch(om, c[sel], dp), dd[sel], pdr.astype(np.float64))
        assert ill.mean() <= ILLCOND_MAX
        plog(f"{tag}_given_pdf_err_over_tol",
             (np.abs(pdw[sel][~ill] - pdr[~ill]) / (PDF_ATOL + PDF_RTOL * np.abs(pdr[~ill]))).max(initial=0.0), 1.0)
        np.testing.assert_allclose(pdw[sel][~ill], pdr[~ill], rtol=PDF_RTOL, atol=PDF_ATOL)
        served += len(sel)
    assert served + int((node == leaves[3]).sum()) == nq


@pytest.mark.gpu
@pytest.mark.parametrize("name,K,cap", [(n, K, cap) for n in ("clones", "pairs", "steep") for K in (16, 128)
                                        for cap in (40, 0)])
def test_product_constructed(pkg, oracle, synth, gpu, plog, name, K, cap):
    """Product sampling (guide_product_kernel and its full-K fallback) on the
    constructed families, set up as test_product_matches_oracle: h and the
    index bit for bit, product rows 1e-6 / 1e-5 rel, plain-conditional rows
    the guide's 1e-5 / 1e-4 rel."""
    import torch
    mix, om, ref, memo = device_case(pkg, oracle, name, K)
    nq = 600
    c, u = ref["c"][:nq], ref["u"][:nq]
    B, M = 2, 4
    bw, bmean, bcov = synth.bsdf_table(B, M)
    F = synth.shading_frames(nq)
    mat = ((np.arange(nq) % (B + 1)) - 1).astype(np.int32)          # -1: no learned BSDF
    if "product" not in memo:
        dr, pr, cr, hr = oracle.guide_product_batch(om, c, u, mat, F, bw, bmean, bcov)
        at = lambda dp: oracle.guide_product_batch(om, c, u, mat, F, bw, bmean, bcov, dgiven=dp)[1]
        nonunit = non_unit(dr)
        memo["product"] = {"d": dr, "pdf": pr, "comp": cr, "h": hr, "nonunit": nonunit,
                           "ill": ill_conditioned(at, dr, at(dr).astype(np.float64)) & ~nonunit}
    pref = memo["product"]
    tag = f"product_{name}_K{K}_cap{cap}"
    check_exclusions(pref, plog, tag)
    hr = pref["h"]
    prod, cond, bsdf_only = hr == np.float32(0.3), hr == np.float32(0.5), hr == 1.0
    assert prod.sum() + cond.sum() + bsdf_only.sum() == nq
    if name == "steep" and K == 16:
        assert prod.any() and cond.any() and bsdf_only.any()       # all three h classes
    mix.set_guide_capacity(cap)
    table = pkg.BsdfTable(bw, bmean, bcov, device=gpu)
    d, pdf, comp, h = mix.guide_product(planes(gpu, c), planes(gpu, u), table, torch.from_numpy(mat).to(gpu),
                                        planes(gpu, F))
    torch.cuda.synchronize()
    got = (np.stack([x.cpu().numpy() for x in d], 1), pdf.cpu().numpy(), comp.cpu().numpy())
    hg = h.cpu().numpy()
    plog(f"{tag}_heuristic_mismatches", int((hg != hr).sum()), 0, product_frac=float(prod.mean()))
    np.testing.assert_array_equal(hg, hr)
    np.testing.assert_array_equal(got[2], pref["comp"])
    compare(plog, tag + "_prod", got, pref, rows=prod, d_atol=PROD_D_ATOL, pdf_rtol=PROD_PDF_RTOL,
            pdf_atol=PROD_PDF_ATOL)
    compare(plog, tag + "_cond", got, pref, rows=cond)
    assert (got[2][bsdf_only] == -1).all() and (got[1][bsdf_only] == 0).all()
