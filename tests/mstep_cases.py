"""Constructed inputs for one stepwise M-step (mstep.hip against or_mstep_f64):
mixture parameters, the stepwise state and the sufficient statistics, built in
numpy so that every branch of mstep_component is reached on purpose, plus the
helpers that load a case into the CPU oracle and measure the oracle's own
movement under a perturbed alpha (the reference band).  No GPU here: the GPU
tests (test_gpu_mstep_edges.py) and the CPU tests of the construction itself
(test_mstep_cases.py) both import this module.

Component k belongs to family FAMILIES[(7 k + k // 64) % 10], which puts
every family into every 64-lane workgroup of mstep_spread_kernel and into the
padded tail.  Each component has a target tangent mean mu (5) and a target
5x5 matrix S; its statistics are W, M = W mu, C = W (S + mu mu^T):

  ord       W in [0.5, 2], |mu[3:5]| <= 1, S SPD          the common path
  dead      mixture weight 0 before the step               in.w == 0
  weak      W = 0 and sgW = 0 (sgM, sgC non-zero)          invW infinite
  pi_over   |mu[3:5]| = 4.0 or pi (1 + 1e-12); at it == 0   embedded mean all 0
            also exactly the double pi (the >= itself)
  pi_under  |mu[3:5]| = pi (1 - 1e-9)                      the antipode
  tiny      |mu[3:5]| in {0, 1e-17, 1e-9, 1e-5, 1e-3}      every sinc_pi_d band
  indef     mu = 0, eig S = 1e-2 [1, .5, .25, .125, -1e-3] killed without priors
  nearsing  mu = 0, smallest eigenvalue 1e-2 NEARSING_LAM  pd_test_keep / Jacobi
  bigW      W = 1e6                                        normalisation scaling
  smallW    W = 1e-30                                      tiny finite invW

The stepwise state (it > 0 blends (1 - eta) of it) is the statistics scaled
per component by independent factors: sgW = a W, sgM = b M, sgC = c C with
a, b in [0.8, 1.2] and c in [2, 2.5], so the blended mean and covariance
depend on eta (with sgW = c W they would not).  c >= 2 keeps
gC - gM gM^T / gW positive definite for S SPD: it equals
W [g S + (g - B^2 / A) mu mu^T] with A, B, g the blended factors, and
g >= B^2 / A for every eta in [0, 1].  Two exceptions, both so that a
decision cannot hang on the last bit of eta (the device's pow and libm's may
differ there):
  * pi_over, pi_under and tiny use b = a: their tangent length is the point
    of the family and must come out of the blend as constructed;
  * nearsing at it > 0 keeps its near-zero eigenvalue on one coordinate axis
    (the other four rotated among themselves): scaling by the blend factors
    then preserves its sign exactly.  At it == 0 (eta == 1 on both sides,
    every operation shared) the rotation is full and rounding decides, as in
    test_mstep_pd_kill_matches_oracle.
"""
import numpy as np

FAMILIES = ("ord", "dead", "weak", "pi_over", "pi_under", "tiny", "indef", "nearsing", "bigW", "smallW")
FAM = {n: i for i, n in enumerate(FAMILIES)}
NEARSING_LAM = (1e-12, 1e-15, 1e-16, 0.0, -1e-16, -1e-15, -1e-12)
TINY_LEN = (0.0, 1e-17, 1e-9, 1e-5, 1e-3)
PI_OVER_LEN = (4.0, np.pi * (1.0 + 1e-12))
# it == 0 only (eta == 1, every operation shared with the oracle): a tangent
# mean that comes out of the M-step's own arithmetic as exactly the double pi
PI_OVER_LEN_IT0 = (np.pi, np.pi * (1.0 + 1e-12), 4.0)
PI_UNDER_LEN = np.pi * (1.0 - 1e-9)
INDEF_EIG = 1e-2 * np.array([1.0, 0.5, 0.25, 0.125, -1e-3])
N_TOTAL = 1000
# scalars of get_state / set_state (sdmm_device.h SC_*)
HTW, SGH, NORM, IT, ALPHA, NI, DECP, CUT, STATUS = range(9)
STATE_F64 = ("T", "sgW", "sgM", "sgC", "heuristicTotalWeight", "sgH")
# (it, cutoff, decrease_prior, priors) of the GPU tests; the last one is an
# addition: eta == 1 and no priors, where rounding decides the nearsing kills
STEP_CASES = ((0, 32, 1, True), (3, 32, 1, True), (3, 32, 0, True), (3, 32, 1, False), (40, 32, 1, True),
              (36, 40, 1, True), (0, 32, 1, False))


def family_of(K):
    k = np.arange(K)
    return (7 * k + k // 64) % 10


def _rot(rng, n):
    q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    return q


def _sym(a):
    return (a + np.swapaxes(a, -1, -2)) / 2


def _spd(rng):
    q = _rot(rng, 5)
    return _sym(q @ np.diag(10.0 ** rng.uniform(-3.0, -1.0, 5)) @ q.T)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def mean_from_stats(M, W, wsum):
    """The tangent-mean entry mstep_component forms from statistics M, W at
    it == 0 (eta == 1: gM = M, gW = W, hTW = wsum), operation for operation."""
    inv_tw = 1.0 / wsum
    return (M * inv_tw) * (1.0 / (W * inv_tw))


def stat_for_exact_pi(W, wsum):
    """(M, W') with mean_from_stats(M, W', wsum) == pi exactly: a search over
    the doubles around pi W, and over the doubles just above W where the
    rounding of the chain skips pi for W itself."""
    for _ in range(256):
        M = float(np.pi * W)
        for _ in range(16):
            m = mean_from_stats(M, W, wsum)
            if m == np.pi:
                return M, W
            M = float(np.nextafter(M, np.inf if m < np.pi else -np.inf))
        W = float(np.nextafter(W, np.inf))
    raise AssertionError("no statistic gives exactly pi")


def compact_stats(H, wsum, W, M, C):
    K = W.shape[0]
    low = np.stack([C[:, i, j] for i in range(5) for j in range(i + 1)], 1)
    return np.concatenate([[H, wsum], W, M.reshape(K * 5), low.reshape(K * 15)])


def full_stats(compact, K):
    from test_gpu_parity import _full_stats
    return _full_stats(np.asarray(compact, np.float64), K)


def build_case(K, it, *, priors=True, decrease_prior=True, cutoff=32, seed=0, families=None):
    """Everything both sides of one M-step need (module docstring).  families:
    an int array overriding family_of(K) (all_killed_case)."""
    rng = np.random.default_rng([seed, K])
    fam = family_of(K) if families is None else np.asarray(families)
    member = np.zeros(K, int)
    for f in range(10):
        idx = np.flatnonzero(fam == f)
        member[idx] = np.arange(idx.size)
    is_ = lambda *names: np.isin(fam, [FAM[n] for n in names])

    # ---- mixture parameters before the step
    w0 = rng.uniform(0.5, 1.5, K)
    w0[is_("dead")] = 0.0
    w0 = w0 / w0.sum()
    mean0 = np.concatenate([rng.uniform(0.2, 0.8, (K, 3)), _unit(rng.normal(size=(K, 3)))], 1)
    cov0 = np.stack([_spd(rng) for _ in range(K)])

    # ---- targets: tangent mean mu and S
    length = rng.uniform(0.0, 1.0, K)
    over = PI_OVER_LEN_IT0 if it == 0 else PI_OVER_LEN
    for k in np.flatnonzero(is_("pi_over")):
        length[k] = over[member[k] % len(over)]
    length[is_("pi_under")] = PI_UNDER_LEN
    for k in np.flatnonzero(is_("tiny")):
        length[k] = TINY_LEN[member[k] % 5]
    phi = rng.uniform(0.0, 2.0 * np.pi, K)
    exact_pi = is_("pi_over") & (length == np.pi)
    phi[exact_pi] = 0.0                      # (pi, 0): sqrt(pi * pi + 0) == pi
    mu = np.concatenate([rng.uniform(0.2, 0.8, (K, 3)), (length * np.cos(phi))[:, None],
                         (length * np.sin(phi))[:, None]], 1)
    mu[is_("indef", "nearsing")] = 0.0
    S = np.stack([_spd(rng) for _ in range(K)])
    for k in np.flatnonzero(is_("indef")):
        q = _rot(rng, 5)
        S[k] = _sym(q @ np.diag(INDEF_EIG) @ q.T)
    for k in np.flatnonzero(is_("nearsing")):
        lam = NEARSING_LAM[member[k] % len(NEARSING_LAM)]
        if it == 0:
            q = _rot(rng, 5)
            S[k] = _sym(q @ np.diag(1e-2 * np.array([1.0, 0.5, 0.25, 0.125, lam])) @ q.T)
        else:
            q4 = _rot(rng, 4)
            blk = _sym(q4 @ np.diag(1e-2 * np.array([1.0, 0.5, 0.25, 0.125])) @ q4.T)
            ax = int(rng.integers(5))
            rest = [i for i in range(5) if i != ax]
            S[k] = 0.0
            S[k][np.ix_(rest, rest)] = blk
            S[k][ax, ax] = 1e-2 * lam

    # ---- statistics
    W = rng.uniform(0.5, 2.0, K)
    W[is_("bigW")] = 1e6
    W[is_("smallW")] = 1e-30
    W[is_("weak")] = 0.0
    M = W[:, None] * mu
    Cs = _sym(W[:, None, None] * (S + mu[:, :, None] * mu[:, None, :]))
    wsum = 1.25 * float(W.sum())
    H = 0.2 * float(W.sum())
    for k in np.flatnonzero(exact_pi):
        M[k, 3], W[k] = stat_for_exact_pi(float(W[k]), wsum)
    compact = compact_stats(H, wsum, W, M, Cs)

    # ---- stepwise state
    a = rng.uniform(0.8, 1.2, K)
    b = rng.uniform(0.8, 1.2, K)
    c = rng.uniform(2.0, 2.5, K)
    same = is_("pi_over", "pi_under", "tiny")
    b[same] = a[same]
    sgW = a * W
    sgM = b[:, None] * M
    sgC = c[:, None, None] * Cs
    for k in np.flatnonzero(is_("weak")):
        sgM[k] = rng.uniform(-0.1, 0.1, 5)
        sgC[k] = 0.1 * _spd(rng)
    T = rng.uniform(0.5, 1.5, K) * wsum
    scalars = np.zeros(9)
    scalars[HTW] = 0.9 * wsum
    scalars[SGH] = 0.17 * wsum
    scalars[NORM] = float(np.float32(0.7))
    scalars[IT] = float(it)
    scalars[ALPHA] = float(np.float32(0.9))
    scalars[NI] = float(np.float32(6e-5))
    scalars[DECP] = 1.0 if decrease_prior else 0.0
    scalars[CUT] = float(cutoff)
    scalars[STATUS] = 1.0
    bp = np.zeros((K, 5, 5), np.float32)
    bd = np.zeros((K, 3, 3), np.float32)
    if priors:
        for k in range(K):
            r = _rot(rng, 3)
            u = rng.uniform(0.5, 2.0, 5)
            bp[k, :3, :3] = _sym(r @ np.diag(1e-4 * u[:3]) @ r.T)
            bp[k, 3, 3], bp[k, 4, 4] = 1e-5 * u[3], 1e-5 * u[4]
            n = mean0[k, 3:6]
            bd[k] = 1e-6 * n[:, None] * n[None, :]
    state = {"scalars": scalars, "T": T, "sgW": sgW, "sgM": sgM.reshape(-1).copy(),
             "sgC": sgC.reshape(-1).copy(), "bpriors": bp.reshape(-1).copy(), "bdepth": bd.reshape(-1).copy()}
    return {"K": K, "it": it, "family": fam, "member": member, "length": length, "priors": priors,
            "weights": w0.astype(np.float32), "mean": mean0.astype(np.float32), "cov": cov0.astype(np.float32),
            "state": state, "stats": compact, "stats_full": full_stats(compact, K), "n_total": N_TOTAL}


def all_killed_case(K, it, **kw):
    """Every component indef, no priors: all weights and the CDF come out 0
    (sum == 0, fs == 0 in mstep_finish)."""
    kw["priors"] = False
    return build_case(K, it, families=np.full(K, FAM["indef"]), **kw)


def zero_sum_stats(case):
    """The case's statistics with stats[1] == 0 and every other entry non-zero."""
    z = np.array(case["stats"], np.float64)
    z[z == 0.0] = 1.0
    z[1] = 0.0
    return z


def members(case, name):
    return np.flatnonzero(case["family"] == FAM[name])


# ---------------------------------------------------------------------------
# the oracle side

def mix_fields(oracle):
    return tuple(oracle.MIX_FIELDS)


def params_of(oracle, m):
    """A get_params()-shaped dict (copies) of an oracle.Mixture."""
    p = {n: np.array(getattr(m, n)) for n in oracle.MIX_FIELDS}
    p["valid"] = m.valid.copy()
    p["normalization"] = float(m.s.normalization)
    return p


def oracle_initial_params(oracle, case):
    """What set_params leaves (set_all_kernel: MVTN::set of the fp64-widened
    float means and covariances, then configure()), from the oracle's own
    set_component(mode=1) + configure: the CPU tests' starting point."""
    K = case["K"]
    m = oracle.Mixture(K)
    m.weights[:] = case["weights"]
    for k in range(K):
        m.set_component(k, case["mean"][k].astype(np.float64), case["cov"][k].astype(np.float64), mode=1)
    m.configure()
    p = params_of(oracle, m)
    p["normalization"] = float(case["state"]["scalars"][NORM])
    return p


def load_oracle(oracle, K, params, state, alpha=None):
    """(Mixture, EmState) holding exactly the floats of params (a get_params()
    dict, valid included) and of the stepwise state."""
    m = oracle.Mixture(K)
    m.copy_params_from(params)
    m.valid[:] = params["valid"]
    sc = state["scalars"]
    m.s.normalization = float(np.float32(sc[NORM]))
    st = oracle.EmState(K)
    st.s.iterationsRun = int(sc[IT])
    st.s.decreasePrior = int(sc[DECP] != 0.0)
    st.s.trainingCutoff = int(sc[CUT])
    st.s.alpha = float(sc[ALPHA]) if alpha is None else float(alpha)
    st.s.niPriorMinusOne = float(sc[NI])
    st.s.heuristicTotalWeight = float(sc[HTW])
    st.s.sgH = float(sc[SGH])
    st.d["totalWeight"][:] = state["T"]
    st.d["sgW"][:] = state["sgW"]
    st.d["sgM"][:] = np.asarray(state["sgM"]).reshape(-1)
    st.d["sgC"][:] = np.asarray(state["sgC"]).reshape(-1)
    st.bPriors[:] = np.asarray(state["bpriors"]).reshape(-1)
    st.bDepth[:] = np.asarray(state["bdepth"]).reshape(-1)
    return m, st


def state_of(m, st):
    """The oracle's stepwise state under the names of STATE_F64 (+ the rest)."""
    return {"T": st.d["totalWeight"].copy(), "sgW": st.d["sgW"].copy(), "sgM": st.d["sgM"].copy(),
            "sgC": st.d["sgC"].copy(), "heuristicTotalWeight": np.array([st.s.heuristicTotalWeight]),
            "sgH": np.array([st.s.sgH]), "normalization": np.float32(m.s.normalization),
            "it": int(st.s.iterationsRun)}


def gpu_state_named(st):
    """get_state() under the same names."""
    sc = st["scalars"]
    return {"T": st["T"], "sgW": st["sgW"], "sgM": st["sgM"], "sgC": st["sgC"],
            "heuristicTotalWeight": np.array([sc[HTW]]), "sgH": np.array([sc[SGH]]),
            "normalization": np.float32(sc[NORM]), "it": int(sc[IT]), "status": float(sc[STATUS])}


def run_oracle(oracle, K, params, state, stats_full, n_total, alpha=None):
    """One or_mstep_f64 from (params, state): (return code, params after, state after)."""
    m, st = load_oracle(oracle, K, params, state, alpha)
    rc = oracle.mstep(m, st, stats_full, n_total, accurate=True)
    return rc, params_of(oracle, m), state_of(m, st)


def rel_dist(a, ref):
    """max |a - ref| / max |ref| (0 / 0 = 0: an array that is all zero on both sides)."""
    a, ref = np.asarray(a, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    num, den = float(np.abs(a - ref).max()), float(np.abs(ref).max())
    if den == 0.0:
        return 0.0 if num == 0.0 else float("inf")
    return num / den


def reference_band(oracle, K, params, state, stats_full, n_total):
    """The reference's own movement under alpha (1 +- 2^-40): for each fp64
    state array max over both signs of |a - a'| / max |a|, the same for every
    float output (dict `floats`), and whether any decision moved (`stable`:
    the killed set, the valid flags and the non-finite pattern of every
    output are those of the unperturbed run).  Returns (band, base) with base
    the unperturbed (rc, params, state)."""
    alpha = float(state["scalars"][ALPHA])
    base = run_oracle(oracle, K, params, state, stats_full, n_total)
    band = {n: 0.0 for n in STATE_F64}
    floats = {n: 0.0 for n in oracle.MIX_FIELDS}
    stable = True
    for sgn in (1.0, -1.0):
        rc, p, s = run_oracle(oracle, K, params, state, stats_full, n_total, alpha * (1.0 + sgn * 2.0 ** -40))
        stable &= rc == base[0]
        stable &= np.array_equal(p["weights"] == 0, base[1]["weights"] == 0)
        stable &= np.array_equal(p["valid"], base[1]["valid"])
        for n in STATE_F64:
            band[n] = max(band[n], rel_dist(s[n], base[2][n]))
        for n in oracle.MIX_FIELDS:
            x, y = p[n].astype(np.float64), base[1][n].astype(np.float64)
            fin = np.isfinite(y)
            stable &= np.array_equal(np.isfinite(x), fin)
            if fin.any() and np.abs(y[fin]).max() > 0:
                floats[n] = max(floats[n], float(np.abs(x[fin] - y[fin]).max() / np.abs(y[fin]).max()))
    band["floats"] = floats
    band["stable"] = bool(stable)
    return band, base


# ---------------------------------------------------------------------------
# comparisons shared by the tests

def ulp_distance(a, b):
    """Distance in float32 ulps between finite entries (0 where both are
    non-finite with the same bits; a huge value where only one is finite or
    the non-finite bits differ)."""
    a = np.ascontiguousarray(a, np.float32).reshape(-1)
    b = np.ascontiguousarray(b, np.float32).reshape(-1)
    ia = a.view(np.int32).astype(np.int64)
    ib = b.view(np.int32).astype(np.int64)
    ma = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    mb = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    d = np.abs(ma - mb)
    nf = ~np.isfinite(a) | ~np.isfinite(b)
    d[nf] = np.where(ia[nf] == ib[nf], 0, 1 << 40)
    return d
