"""GPU: the E-step statistics kernels and the EM step at their edges.

estep_stats_kernel (K <= 64), estep_stats_tile_kernel (64 < K <= 128), its
GROUP forms (K <= 256, K <= 512) and the reduce_uncenter kernels against the
fp64 evaluation of the same float parameters (helpers.estep_f64), at
  A. padded K (K < Kp, odd K), tails and nearly empty launches (N < 64, N no
     multiple of the 4-sample tile);
  B. the reference's angle quirks (mvtn.h:152-164) in chosen tile positions;
  C. three EM steps at padded K against the exact EM;
  D. samples with a NaN / Inf coordinate and a finite, non-zero weight.

Mixtures at arbitrary K: uniformHemisphereInit wants K / 8 seed points, so the
mixture is initialised (and for `fitted` run through 3 EM steps) at the next
padded size Kp, its first K components are kept with renormalised weights and
loaded through set_params, and the oracle copies the device's derived arrays.
"""
import numpy as np
import pytest

from helpers import estep_f64, posterior_f64
from test_gpu_parity import RTOL_PARAMS, _exact_em, _full_stats, _param_err

pytestmark = pytest.mark.gpu

STATS_TOL = 1e-6       # of the total weight (test_stats_match_oracle)
NBASE = 4096           # no test runs above this many samples

_cache = {}


def _kp(K):
    return next(k for k in (16, 32, 64, 128, 256, 512) if K <= k)


def family(K):
    return "legacy" if K <= 64 else "tile" if K <= 128 else "group2" if K <= 256 else "group4"


def _base(synth, heuristic=False, guards=True):
    key = ("base", heuristic, guards)
    if key not in _cache:
        _cache[key] = synth.em_batch(NBASE, 128, heuristic=heuristic, guards=guards)
    return _cache[key]


def _padded_mixture(pkg, synth, Kp, fitted):
    """Host parameters and hemisphere priors of the Kp-component mixture."""
    key = ("kp", Kp, fitted)
    if key not in _cache:
        b = _base(synth)
        pos, nrm = synth.model_seed_points(b, Kp)
        mix = pkg.SDMM(Kp)
        mix.init_hemisphere(pos, nrm, synth.DEPTH_PRIOR, synth.SPATIAL_DISTANCE, synth.SEED_MODEL)
        st = mix.get_state()
        if fitted:
            mix.optimize(pkg.DeviceSamples.from_numpy(b["x"], b["w"], b["hpdf"], b["is_diffuse"]), 3)
        p = mix.get_params()
        _cache[key] = {"weights": p["weights"].copy(), "mean": p["mean"].copy(), "cov": p["cov"].copy(),
                       "bpriors": st["bpriors"].reshape(Kp, 25).copy(), "bdepth": st["bdepth"].reshape(Kp, 9).copy()}
    return _cache[key]


def sliced(pp, K):
    """First K components, weights renormalised (fp64 sum, rounded once)."""
    w = pp["weights"][:K].astype(np.float64)
    return (w / w.sum()).astype(np.float32), pp["mean"][:K].copy(), pp["cov"][:K].copy()


def _mixture(pkg, oracle, synth, K, fitted, perturb_dropped=False):
    """(device mixture, its exported parameters, the oracle's copy, padded host parameters)."""
    pp = _padded_mixture(pkg, synth, _kp(K), fitted)
    if perturb_dropped:
        # other (valid) parameters in the components that the slice drops
        pp = {k: v.copy() for k, v in pp.items()}
        pp["weights"][K:] *= 3.0
        pp["mean"][K:, :3] += 0.25
        pp["cov"][K:] *= 2.0
    w, mean, cov = sliced(pp, K)
    mix = pkg.SDMM(K)
    mix.set_params(w, mean, cov)
    p = mix.get_params()
    om = oracle.Mixture(K)
    om.copy_params_from(p)
    om.valid[:] = p["valid"]
    return mix, p, om, pp


def stats_scale(exact, w):
    """The total weight; at very small N it can be tiny (or 0 with the guard
    rows), so never below the sum of the finite |w|."""
    fin = np.isfinite(w)
    return max(abs(float(exact[1])), float(np.abs(w[fin].astype(np.float64)).sum()))


def stats_err(a, b, scale):
    with np.errstate(invalid="ignore"):
        d = np.abs(a - b)
    return float(np.where(np.isfinite(d), d, np.inf).max() / scale)


def _gpu_stats(pkg, gpu, mix, K, ds, guard=8, sentinel=-7.0):
    """estep_stats into a buffer with `guard` sentinel entries behind it:
    (compact vector, guard entries after the call)."""
    import torch
    n = pkg.stats_len(K)
    assert n == 2 + 21 * K
    st = torch.full((n + guard,), sentinel, dtype=torch.float64, device=gpu)
    mix.estep_stats(ds, st)
    torch.cuda.synchronize()
    out = st.cpu().numpy()
    return out[:n], out[n:]


# ---- A: padded K, tails, nearly empty launches ----------------------------
# (K, N, heuristic, fitted): every kernel family meets every N, every K at
# least two N, one heuristic case per family
CASES_A = [
    # estep_stats_kernel: LPS 8 (K <= 16), 16 (K <= 32), 32 (K <= 64)
    (1, 1, False, False), (1, 63, False, True), (2, 3, False, True), (2, 257, False, False),
    (15, 5, False, False), (15, 1001, False, True), (17, 63, False, False), (17, 65, False, True),
    (33, 1, False, True), (33, 65, False, False), (63, 3, False, False), (63, 257, False, True),
    (63, 1001, True, True),
    # estep_stats_tile_kernel<4, *>
    (65, 1, False, False), (65, 65, False, True), (65, 1001, False, False), (72, 3, False, True),
    (72, 63, False, False), (72, 257, True, True), (127, 5, False, True), (127, 257, False, False),
    (127, 1001, False, True),
    # GROUP <2, 2, true>
    (129, 1, False, True), (129, 5, False, False), (129, 65, False, True), (129, 1001, False, False),
    (200, 3, False, False), (200, 63, False, True), (200, 257, False, False), (200, 1001, True, True),
    # GROUP <4, 2, true>
    (257, 1, False, False), (257, 65, False, False), (257, 1001, False, True), (300, 3, False, True),
    (300, 63, True, True), (300, 257, False, False), (511, 5, False, False), (511, 63, False, True),
    (511, 1001, False, True),
]


def test_cases_a_cover_every_family_and_size():
    ns = {1, 3, 5, 63, 65, 257, 1001}
    ks = {1, 2, 15, 17, 33, 63, 65, 72, 127, 129, 200, 257, 300, 511}
    assert {c[0] for c in CASES_A} == ks
    for fam in ("legacy", "tile", "group2", "group4"):
        assert {c[1] for c in CASES_A if family(c[0]) == fam} == ns, fam
        assert any(c[2] for c in CASES_A if family(c[0]) == fam), fam
    for k in ks:
        assert len({c[1] for c in CASES_A if c[0] == k}) >= 2, k


@pytest.mark.parametrize("K,N,heuristic,fitted", CASES_A)
def test_stats_padded_k_and_tails(pkg, oracle, synth, gpu, plog, K, N, heuristic, fitted):
    """estep_stats at K < Kp and short batches against estep_f64 of the same
    float parameters: within 1e-6 of the total weight (scaled by
    max(|weightSum|, sum of the finite |w|): at N = 1..5 the total weight is a
    single sample's), weightSum at rtol 1e-6.  A case past 1e-6 where the fp32
    oracle (accurate=True) is past it too is ill-conditioned input, bounded at
    4 x the oracle's error + 1e-6 and recorded (`relative_bound` in the log).
    The compact vector uses exactly 2 + 21 K entries, all finite.

    Realised on the MI355X: the 39 cases sit at 3.6e-9 .. 1.3e-7 (largest:
    K = 129, N = 1, one sample's rounding against its own weight); the fp32
    oracle at 2.8e-9 .. 8.9e-7.  No case took the relative bound."""
    b = _base(synth, heuristic)
    x, w, hp, isd = b["x"][:, :N], b["w"][:N], b["hpdf"][:N], b["is_diffuse"][:N]
    mix, p, om, _ = _mixture(pkg, oracle, synth, K, fitted)
    ds = pkg.DeviceSamples.from_numpy(x, w, hp, isd)
    compact, guard = _gpu_stats(pkg, gpu, mix, K, ds)
    assert (guard == -7.0).all(), "estep_stats wrote past 2 + 21 K entries"
    assert np.isfinite(compact).all()
    got = _full_stats(compact, K)
    exact = estep_f64(p, x, w, hp, isd)
    ref = oracle.calculate_stats(om, oracle.Samples(x, w, hp, isd), accurate=True)
    scale = stats_scale(exact, w)
    eg, eo = stats_err(got, exact, scale), stats_err(ref, exact, scale)
    relative = eg > STATS_TOL and eo > STATS_TOL
    bound = 4 * eo + STATS_TOL if relative else STATS_TOL
    print(f"A K={K} N={N} h={heuristic} fitted={fitted}: stats err gpu {eg:.2e} oracle-fp32 {eo:.2e} "
          f"bound {bound:.2e}{' (relative)' if relative else ''}")
    plog("stats_edges_rel_err_vs_fp64", eg, bound, oracle_fp32_err=eo, relative_bound=bool(relative),
         family=family(K))
    np.testing.assert_allclose(got[1], exact[1], rtol=1e-6)
    assert eg <= bound, (eg, eo)


@pytest.mark.parametrize("K,N", [(15, 65), (72, 257), (129, 63), (200, 1001), (300, 257), (511, 65)])
def test_stats_pad_columns_do_not_leak(pkg, oracle, synth, gpu, K, N):
    """The same K components cut from two Kp-component mixtures that differ in
    the dropped components K .. Kp - 1 (weights, positions, covariances), on
    two handles: the statistics are bitwise equal, so nothing a pad column
    (k >= K) holds -- whatever a fresh handle's padded record contains --
    reaches a real column through the kernels or the reduction."""
    b = _base(synth)
    ds = pkg.DeviceSamples.from_numpy(b["x"][:, :N], b["w"][:N], b["hpdf"][:N], b["is_diffuse"][:N])
    out = []
    for perturb in (False, True):
        mix, p, _, pp = _mixture(pkg, oracle, synth, K, True, perturb_dropped=perturb)
        out.append((_gpu_stats(pkg, gpu, mix, K, ds)[0], p, pp))
    assert not np.array_equal(out[0][2]["mean"][K:], out[1][2]["mean"][K:])     # the dropped ones differ
    for name in ("weights", "mean", "cov"):
        np.testing.assert_array_equal(out[0][1][name], out[1][1][name])
    np.testing.assert_array_equal(out[0][0], out[1][0])


# ---- B: the angle quirks through the statistics kernels -------------------
ORDINARY, NEAR_ANTIPODE, ON_MEAN, ANTIPODE, ZERO_DIR = range(5)


def quirk_batch(mean, base_x, K, seed=11):
    """N = 8 K - 1 rows of `base_x` with quirk directions written into chosen
    rows (4-sample tiles start at multiples of 4: every chunk is a multiple
    of 64 samples), each at the spatial mean of its target k = 4 i + 3 (never
    slot 0 of a lane's components, test_rare_angle_every_lane_slot):
      [0, 4K)  rows 3 mod 4: 7.5e-4..8.5e-4 rad from k's antipode -- the only
               odd sample of its tile is t = 3;
      [4K, 5K) every row near-antipodal (the redo replaces all four);
      [5K, 6K) rows 1 mod 4: the stored float mean direction itself;
      [6K, 7K) rows 2 mod 4: -(1 + 2^-18) n, just past the antipode: c <= -1
               and the log map fails in every arithmetic.  (At -n itself
               c = -|n|^2 falls on either side of -1 by the rounding of the
               stored n, differently in fp32 and fp64: the fp32 oracle then
               disagrees with fp64 on whole rows, eo rises from ~5e-8 to
               ~6e-4 and the bound loosens for every row.)
      [7K, 8K - 4) rows 0 mod 4: d = 0;
      row 8K - 2: near-antipodal, sample t = 2 of the last, partial tile
               (3 samples).
    Returns (x, class per row, target per row)."""
    N = 8 * K - 1
    x = base_x[:, :N].copy()
    mu = mean.astype(np.float64)
    rng = np.random.default_rng(seed)
    cls = np.full(N, ORDINARY)
    i = np.arange(N)
    cls[(i < 4 * K) & (i % 4 == 3)] = NEAR_ANTIPODE
    cls[(i >= 4 * K) & (i < 5 * K)] = NEAR_ANTIPODE
    cls[(i >= 5 * K) & (i < 6 * K) & (i % 4 == 1)] = ON_MEAN
    cls[(i >= 6 * K) & (i < 7 * K) & (i % 4 == 2)] = ANTIPODE
    cls[(i >= 7 * K) & (i < 8 * K - 4) & (i % 4 == 0)] = ZERO_DIR
    cls[8 * K - 2] = NEAR_ANTIPODE
    tgt = np.full(N, -1)
    for c in (NEAR_ANTIPODE, ON_MEAN, ANTIPODE, ZERO_DIR):
        rows = np.flatnonzero(cls == c)
        tgt[rows] = 4 * (np.arange(rows.size) % (K // 4)) + 3
    for r in np.flatnonzero(cls != ORDINARY):
        k = tgt[r]
        x[0:3, r] = mean[k, 0:3]
        if cls[r] == NEAR_ANTIPODE:
            n = mu[k, 3:6] / np.linalg.norm(mu[k, 3:6])
            t = np.cross(n, [0.0, 0.0, 1.0] if abs(n[2]) < 0.9 else [1.0, 0.0, 0.0])
            t /= np.linalg.norm(t)
            dl = rng.uniform(7.5e-4, 8.5e-4)
            x[3:6, r] = (-np.cos(dl) * n + np.sin(dl) * t).astype(np.float32)
        elif cls[r] == ON_MEAN:
            x[3:6, r] = mean[k, 3:6]
        elif cls[r] == ANTIPODE:
            x[3:6, r] = (-(1.0 + 2.0 ** -18) * mu[k, 3:6]).astype(np.float32)
        else:
            x[3:6, r] = 0.0
    return x, cls, tgt


def check_quirk_batch_bites(p, x, w, cls, tgt, exact, eo):
    """The CPU side of B: the quirk rows matter.  The targeted component holds
    a substantial share of the near-antipodal rows, and an fp64 evaluation
    WITHOUT the sin < 1e-3 quirk is further from the real one than ten times
    the bound the GPU is held to.  Returns that distance."""
    near = np.flatnonzero(cls == NEAR_ANTIPODE)
    post = posterior_f64(p, x[:, near])
    share = float(np.median(post[np.arange(near.size), tgt[near]]))
    assert share > 0.05, share
    # d == 0 fails every log map; past the antipode the target's fails
    assert (posterior_f64(p, x[:, cls == ZERO_DIR]) == 0).all()
    anti = np.flatnonzero(cls == ANTIPODE)
    assert (posterior_f64(p, x[:, anti])[np.arange(anti.size), tgt[anti]] == 0).all()
    plain = estep_f64(p, x, w, quirk=False)
    dq = stats_err(plain, exact, stats_scale(exact, w))
    assert dq > 10 * (4 * eo + STATS_TOL), (dq, eo)
    return dq


@pytest.mark.parametrize("K", [16, 72, 128, 256, 512])
def test_stats_quirk_directions(pkg, oracle, synth, gpu, plog, K):
    """The reference's angle quirks in the statistics kernels -- the legacy
    kernel's pair_pdf_stats / dfail() (K = 16) and the tile kernels' RARE redo
    (detector, angle_over_sin_tile_d<true>, the per-sample replacement) -- on
    an unfitted mixture, where a quirk row moves the statistics by O(1)
    (quirk_batch: the rows and their tile positions).  Against estep_f64, with
    the fp32 oracle's own distance eo from it as the yardstick:
    eg <= 4 eo + 1e-6 (no flat 1e-6 here: near the antipode theta / sin(theta)
    amplifies fp32 rounding, helpers.explained_rows).

    Realised on the MI355X, eg / eo (the bound 4 eo + 1e-6; the fp64
    evaluation without the quirk sits dq away), of the total weight:
      K = 16   4.06e-8 / 2.55e-8  (1.10e-6; dq 1.17)
      K = 72   6.07e-8 / 8.07e-8  (1.32e-6; dq 1.37e-1)
      K = 128  2.35e-8 / 4.69e-8  (1.19e-6; dq 1.28e-1)
      K = 256  4.64e-8 / 1.07e-5  (4.38e-5; dq 6.80e-2)
      K = 512  3.99e-8 / 6.59e-6  (2.74e-5; dq 2.87e-2)
    With the redo forced onto pair_qt_fast<false> the four tile / GROUP cases
    fail (the legacy kernel has no redo)."""
    b = _base(synth, guards=False)
    mix, p, om, _ = _mixture(pkg, oracle, synth, K, fitted=False)
    x, cls, tgt = quirk_batch(p["mean"], b["x"], K)
    N = x.shape[1]
    w = b["w"][:N]
    exact = estep_f64(p, x, w)
    ref = oracle.calculate_stats(om, oracle.Samples(x, w), accurate=True)
    scale = stats_scale(exact, w)
    eo = stats_err(ref, exact, scale)
    dq = check_quirk_batch_bites(p, x, w, cls, tgt, exact, eo)
    compact, guard = _gpu_stats(pkg, gpu, mix, K, pkg.DeviceSamples.from_numpy(x, w))
    assert (guard == -7.0).all() and np.isfinite(compact).all()
    got = _full_stats(compact, K)
    eg = stats_err(got, exact, scale)
    print(f"B K={K} N={N}: stats err gpu {eg:.3e} oracle-fp32 {eo:.3e} bound {4 * eo + STATS_TOL:.3e} "
          f"no-quirk fp64 {dq:.3e}")
    plog("stats_quirk_rel_err_vs_fp64", eg, 4 * eo + STATS_TOL, oracle_fp32_err=eo, no_quirk_fp64_dist=dq,
         family=family(K))
    np.testing.assert_allclose(got[1], exact[1], rtol=1e-6)
    assert eg <= 4 * eo + STATS_TOL, (eg, eo)


# ---- C: EM steps at padded K ----------------------------------------------
@pytest.mark.parametrize("K", [15, 72, 129, 300])
def test_em_padded_k(pkg, oracle, synth, gpu, plog, K):
    """Three optimize() steps at K < Kp, N = 4096, against the exact EM (fp64
    E-step + the oracle's M-step) at the 1e-4 of test_em_matches_oracle, with
    the iteration counter, the set of live weights and the finiteness of every
    exported parameter checked after each step.  The stepwise state's scalars
    (normalisation, heuristic totals) belong to the whole Kp-component mixture
    and do not slice, so both sides start from the constructor state with the
    same parameters -- and the first K components' hemisphere priors (bPriors,
    bDepth, which are per component) copied in.

    Realised on the MI355X: 4.6e-7 .. 3.9e-6 over the three steps (the fp32
    oracle's E-step: 3.9e-6 .. 5.8e-4, the latter at K = 300)."""
    b = _base(synth)
    N = NBASE
    mix, p, om, pp = _mixture(pkg, oracle, synth, K, fitted=False)
    st = mix.get_state()
    st["bpriors"] = pp["bpriors"][:K].reshape(-1).copy()
    st["bdepth"] = pp["bdepth"][:K].reshape(-1).copy()
    mix.set_state(st)
    xm = oracle.Mixture(K)
    xm.copy_params_from(p)
    xm.valid[:] = p["valid"]
    states = []
    for _ in range(2):
        s = oracle.EmState(K)
        s.bPriors[:] = st["bpriors"]
        s.bDepth[:] = st["bdepth"]
        states.append(s)
    ost, xst = states
    ds = pkg.DeviceSamples.from_numpy(b["x"], b["w"], b["hpdf"], b["is_diffuse"])
    os_ = oracle.Samples(b["x"], b["w"], b["hpdf"], b["is_diffuse"])
    for it in range(3):
        mix.optimize(ds)
        assert oracle.optimize(om, ost, os_, accurate=True) == 1
        _exact_em(oracle, xm, xst, b, 1)
        q = mix.get_params()
        for name, v in q.items():
            assert np.isfinite(v).all(), name
        o = {k: getattr(om, k) for k in ("weights", "mean", "cov")}
        e = {k: getattr(xm, k) for k in ("weights", "mean", "cov")}
        eg, eo = _param_err(q, e), _param_err(o, e)
        print(f"C K={K} it={it + 1}: param err vs exact: gpu {eg:.2e} oracle-fp32-E {eo:.2e}")
        plog("em_padded_k_param_rel_err_vs_exact", eg, RTOL_PARAMS, iteration=it + 1, oracle_fp32_err=eo)
        assert int(mix.get_state()["scalars"][3]) == it + 1
        np.testing.assert_array_equal(q["weights"] > 0, om.weights > 0)
        assert eg <= RTOL_PARAMS


# ---- D: non-finite coordinates with finite weights ------------------------
def poisoned_batch(b, N=1001):
    """Ordinary samples with a NaN position at rows 1::97, a NaN direction at
    2::97, a +Inf position coordinate at 3::97 and a NaN position in the last
    row (N = 1001: the only sample of the final, partial tile), all with
    finite non-zero weights.  Returns (x, w, the rows)."""
    x = b["x"][:, :N].copy()
    w = b["w"][:N].copy()
    rows = np.zeros(N, bool)
    x[0:3, 1::97] = np.nan
    x[3:6, 2::97] = np.nan
    x[0, 3::97] = np.inf
    x[0:3, N - 1] = np.nan
    for a in (1, 2, 3):
        rows[a::97] = True
    rows[N - 1] = True
    fix = rows & ~(np.isfinite(w) & (w != 0))
    w[fix] = 1.5
    return x, w, rows


@pytest.mark.parametrize("K,heuristic", [(16, False), (128, False), (256, False), (512, False),
                                         (16, True), (128, True)])
def test_stats_nonfinite_coordinates(pkg, oracle, synth, gpu, plog, K, heuristic):
    """A sample with a NaN / Inf coordinate and a finite weight: the reference
    checks only the weight (stepwise_tangent.h:445-449), zeroes such a
    sample's posterior (1/sum not finite) and skips it at posterior < 1e-10,
    while sumWeights still counts it.  The kernels formed v = 0 for it and
    then multiplied by its NaN tangent (0 * NaN = NaN, no fast-math): every
    statistic of the lane's components was poisoned.  They now stage such a
    sample as a failed log map (estep.hip dead_sample).  Required: every
    statistic finite, weightSum with those weights in, W / M / C / H equal to
    the same batch with those weights 0 and to estep_f64 within 1e-6 of the
    total weight, and one optimize() step finite and within the EM bound of
    oracle.optimize(accurate=True).  heuristic: half the rows diffuse with an
    hpdf, where such a sample's gamma_h is 0 as well (H must not count it);
    on the unfitted mixture, whose L^-1 has exact zeros, so that the Inf rows
    give 0 * Inf = NaN in the reference too (with a full L^-1 an Inf position
    may instead leave every pdf an exact 0 there and gamma_h = 1).

    Before the fix every case failed: 15 K (K = 16) or 20 K of the 21 K
    per-component statistics were NaN -- all but W.
    Realised after it: statistics 3.6e-9 .. 2.7e-8 from estep_f64, bitwise
    equal to the zero-weighted batch (the staged sample no longer forces the
    redo); the EM step 3.0e-7 (K = 16) .. 3.5e-5 (K = 128, heuristic) from the
    oracle's."""
    b = _base(synth, heuristic)
    x, w, rows = poisoned_batch(b)
    N = w.shape[0]
    hp, isd = (b["hpdf"][:N], b["is_diffuse"][:N]) if heuristic else (None, None)
    assert not heuristic or (isd[rows] != 0).sum() >= 8
    mix, p, om, pp = _mixture(pkg, oracle, synth, K, fitted=not heuristic)
    compact, guard = _gpu_stats(pkg, gpu, mix, K, pkg.DeviceSamples.from_numpy(x, w, hp, isd))
    assert (guard == -7.0).all()
    assert np.isfinite(compact).all(), f"{int((~np.isfinite(compact)).sum())} non-finite statistics"
    got = _full_stats(compact, K)
    w0 = np.where(rows, np.float32(0), w)
    zeroed = _full_stats(_gpu_stats(pkg, gpu, mix, K, pkg.DeviceSamples.from_numpy(x, w0, hp, isd))[0], K)
    with np.errstate(invalid="ignore"):
        exact = estep_f64(p, x, w, hp, isd)
        ref = oracle.calculate_stats(om, oracle.Samples(x, w, hp, isd), accurate=True)
    assert np.isfinite(exact).all() and np.isfinite(ref).all()
    fin = np.isfinite(w)
    wsum = float(w[fin].astype(np.float64).sum())
    np.testing.assert_allclose(got[1], wsum, rtol=1e-6)
    np.testing.assert_allclose(zeroed[1], wsum - float(w[rows].astype(np.float64).sum()), rtol=1e-6)
    scale = stats_scale(exact, w)
    keep = np.ones(got.shape[0], bool)
    keep[1] = False                                    # weightSum differs by design
    ez = stats_err(got[keep], zeroed[keep], scale)
    eg, eo = stats_err(got, exact, scale), stats_err(ref, exact, scale)
    print(f"D K={K} h={heuristic}: stats err vs fp64 gpu {eg:.2e} oracle-fp32 {eo:.2e}; vs zero-weighted rows {ez:.2e}")
    plog("stats_nonfinite_rows_rel_err_vs_fp64", eg, STATS_TOL, oracle_fp32_err=eo, family=family(K))
    plog("stats_nonfinite_rows_vs_zero_weight", ez, STATS_TOL)
    assert ez <= STATS_TOL
    assert eg <= STATS_TOL
    # one EM step on that batch (constructor state on both sides)
    ost = oracle.EmState(K)
    mix.optimize(pkg.DeviceSamples.from_numpy(x, w, hp, isd))
    assert oracle.optimize(om, ost, oracle.Samples(x, w, hp, isd), accurate=True) == 1
    q = mix.get_params()
    for name, v in q.items():
        assert np.isfinite(v).all(), name
    err = _param_err(q, {k: getattr(om, k) for k in ("weights", "mean", "cov")})
    print(f"D K={K} h={heuristic}: one EM step, param err vs oracle.optimize {err:.2e}")
    plog("em_nonfinite_rows_param_rel_err_vs_oracle", err, RTOL_PARAMS)
    assert int(mix.get_state()["scalars"][3]) == 1
    assert err <= RTOL_PARAMS
