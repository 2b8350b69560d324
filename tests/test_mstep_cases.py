"""The constructed M-step cases (mstep_cases.py) on the CPU oracle alone: every
family is present and reaches the branch it was built for, no kill / valid
decision hangs on the last bits of eta, and the reference's own movement
under alpha (1 +- 2^-40) -- the band the GPU tests hold the fp64 state to --
is measured, never hard-coded.  So no test of test_gpu_mstep_edges.py can pass
vacuously."""
import numpy as np
import pytest

import mstep_cases as mc

KS = (72, 200)


@pytest.fixture(scope="module")
def runs(oracle):
    """(K, step case) -> (case, params before, band, (rc, params, state) after), computed once."""
    out = {}
    for K in KS:
        for it, cutoff, decp, priors in mc.STEP_CASES:
            case = mc.build_case(K, it, priors=priors, decrease_prior=bool(decp), cutoff=cutoff)
            p0 = mc.oracle_initial_params(oracle, case)
            band, base = mc.reference_band(oracle, K, p0, case["state"], case["stats_full"], case["n_total"])
            out[(K, it, cutoff, decp, priors)] = (case, p0, band, base)
    return out


def _expected_weak_weight(case, K):
    """decNi / sum as or_mstep_f64 forms it: ni / 3^cut when the prior decreases."""
    sc = case["state"]["scalars"]
    cut = int(min(sc[mc.CUT], sc[mc.IT]))
    return sc[mc.NI] * (1.0 / 3.0 ** cut) if sc[mc.DECP] else sc[mc.NI]


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("step", mc.STEP_CASES, ids=lambda s: "it%d-cut%d-decp%d-%s" % (s[0], s[1], s[2], "on" if s[3] else "off"))
def test_families_reach_their_branches(oracle, runs, K, step):
    it, cutoff, decp, priors = step
    case, p0, band, (rc, p, s) = runs[(K,) + step]
    assert rc == 1 and s["it"] == it + 1
    for name in mc.FAMILIES:
        assert mc.members(case, name).size >= 1, name
    w = p["weights"].astype(np.float64)
    killed = (w == 0) & (p0["weights"] != 0)
    # dead stays dead; the start has exactly the dead family at weight 0
    np.testing.assert_array_equal(np.flatnonzero(p0["weights"] == 0), mc.members(case, "dead"))
    assert (w[mc.members(case, "dead")] == 0).all()
    # pi_over: kept, and the embedded mean is all zeros (position included)
    po = mc.members(case, "pi_over")
    assert not killed[po].any()
    assert (p["mean"][po] == 0).all()
    over = mc.PI_OVER_LEN_IT0 if it == 0 else mc.PI_OVER_LEN
    assert {case["length"][k] for k in po} == set(over)
    if it == 0:
        # the member at exactly pi: the M-step's own arithmetic gives the double pi, and >= zeroes it
        ex = [k for k in po if case["length"][k] == np.pi]
        wsum = case["stats"][1]
        for k in ex:
            Mk = case["stats"][2 + K + 5 * k:2 + K + 5 * k + 5]
            assert mc.mean_from_stats(Mk[3], case["stats"][2 + k], wsum) == np.pi and Mk[4] == 0.0
        assert ex
    # pi_under / tiny: kept, the position is the new mean, every sinc band present at K = 200
    for name in ("pi_under", "tiny", "ord", "bigW", "smallW"):
        assert not killed[mc.members(case, name)].any(), name
    if K == 200:
        assert {case["length"][k] for k in mc.members(case, "tiny")} == set(mc.TINY_LEN)
    # weak: weight decNi / sum, no set (mean and cov those of the start)
    wk = mc.members(case, "weak")
    assert (case["stats"][2 + wk] == 0).all() and (case["state"]["sgW"][wk] == 0).all()
    want = _expected_weak_weight(case, K)
    assert (w[wk] > 0).all() and np.ptp(w[wk]) == 0
    np.testing.assert_array_equal(p["mean"][wk], p0["mean"][wk])
    np.testing.assert_array_equal(p["cov"][wk], p0["cov"][wk])
    # ... and decNi / sum itself, sum rebuilt in fp64 from the blended nW of the state after the step
    nW = s["sgW"] / s["heuristicTotalWeight"][0]
    live = w > 0
    total = float(np.sum(np.where(live, want + nW, 0.0)))
    np.testing.assert_allclose(w[wk], want / total, rtol=2e-6)
    # indef: killed whenever the prior is negligible
    if (not priors) or it == 40:
        assert killed[mc.members(case, "indef")].all()
    # nearsing: both outcomes without priors
    if not priors:
        ns = mc.members(case, "nearsing")
        assert killed[ns].any() and (~killed[ns]).any()
    # finiteness: everything with priors; without them only the overflow of
    # smallW's determinants (the reference's own arithmetic)
    for n in oracle.MIX_FIELDS:
        bad = ~np.isfinite(p[n])
        if priors:
            assert not bad.any(), n
        else:
            rows = np.flatnonzero(bad.reshape(K, -1).any(1))
            assert n in ("detInv", "margDetInv") or rows.size == 0, n
            assert np.isin(rows, mc.members(case, "smallW")).all(), n
            assert not np.isnan(p[n]).any(), n
    for n in mc.STATE_F64:
        assert np.isfinite(s[n]).all(), n


@pytest.mark.parametrize("K", KS)
def test_all_killed_and_zero_sum(oracle, K):
    case = mc.all_killed_case(K, 3)
    p0 = mc.oracle_initial_params(oracle, case)
    rc, p, s = mc.run_oracle(oracle, K, p0, case["state"], case["stats_full"], case["n_total"])
    assert rc == 1
    assert (p["weights"] == 0).all() and (p["cdf"] == 0).all()
    for n in oracle.MIX_FIELDS:
        if n not in ("weights", "cdf"):
            np.testing.assert_array_equal(p[n], p0[n], err_msg=n)
    base = mc.build_case(K, 3)
    z = mc.zero_sum_stats(base)
    assert z[1] == 0 and np.count_nonzero(z) == z.size - 1
    q0 = mc.oracle_initial_params(oracle, base)
    rc, q, t = mc.run_oracle(oracle, K, q0, base["state"], mc.full_stats(z, K), base["n_total"])
    assert rc == 0 and t["it"] == 3
    for n in oracle.MIX_FIELDS:
        np.testing.assert_array_equal(q[n], q0[n], err_msg=n)
    np.testing.assert_array_equal(t["sgC"], base["state"]["sgC"])


@pytest.mark.parametrize("K", KS)
def test_decisions_stable_and_band_measured(oracle, runs, K):
    """No killed-or-kept outcome, valid flag or non-finite pattern changes
    under alpha (1 +- 2^-40) -- a condition on the inputs -- and the band is
    what the arithmetic says: zero at it == 0 (pow(1, -alpha) == 1), a
    few thousand fp64 ulps at it > 0, with the float outputs within an ulp or
    two of where they were."""
    for step in mc.STEP_CASES:
        case, p0, band, base = runs[(K,) + step]
        assert band["stable"], step
        for n in mc.STATE_F64:
            print(f"K={K} {step}: band {n} {band[n]:.3e}")
            if step[0] == 0:
                assert band[n] == 0.0, (step, n)
            else:
                # eta moves by ~ alpha ln(1 + 0.2 it) 2^-40 <= 2e-12 relative
                assert 0.0 < band[n] < 1e-11, (step, n, band[n])
        for n, v in band["floats"].items():
            assert v <= 4 * 2.0 ** -23, (step, n, v)


def test_ulp_distance():
    one = np.float32(1.0)
    up = np.nextafter(one, np.float32(2.0))
    assert mc.ulp_distance([one, 0.0, -0.0, np.inf], [up, -0.0, 0.0, np.inf]).tolist() == [1, 0, 0, 0]
    assert mc.ulp_distance([np.float32(1e-45)], [np.float32(-1e-45)])[0] == 2
    assert mc.ulp_distance([np.inf, np.nan], [-np.inf, 1.0]).min() > 1 << 30
