"""The M-step and MVTN::set on CONSTRUCTED statistics and states (mstep.hip
against or_mstep_f64 / or_component_set), DESIGN.md "Parity: the M-step".

mstep_cases.py builds the inputs (ten families that reach every branch of
mstep_component, all_killed, zero_sum); test_mstep_cases.py proves on the CPU
that they reach them.  Both sides start from the same floats: set_params on
the GPU, get_params() copied into an oracle.Mixture, the stepwise state through
set_state and into the fields of an oracle.EmState.

Bounds (compare_step):
  exact     the killed set, valid, scalars[IT], scalars[STATUS], the bits of
            every non-finite entry, the zero weights; every derived array of
            a component that was not set (dead, killed, weak) is bitwise what
            it was; cdf non-decreasing, its last entry the oracle's float sum;
  it == 0   pow(1, -alpha) == 1 on both sides, every fp64 operation is shared:
            T, sgW, sgM, sgC, heuristicTotalWeight, sgH, cov and mean[:, :3]
            bitwise the oracle's;
  it > 0    each fp64 state array within 4 x the reference band (the
            oracle's own movement under alpha (1 +- 2^-40), measured per case
            by mstep_cases.reference_band: the only operation not shared is
            pow, and 4 x is room for a few ulps of it);
  floats    every MIX_FIELDS array and the normalisation within 1 float ulp of
            the oracle, mean[:, 3:6] and `to` (behind the device's sin / cos)
            within 2.
"""
import ctypes as C

import numpy as np
import pytest

import mstep_cases as mc

pytestmark = pytest.mark.gpu

KS = (15, 64, 65, 72, 129, 200, 512)   # 65: the smallest K above 64 (sdmm_create takes any K in [1, 512])
TWO_ULP = ("mean_dir", "to")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _load(pkg, case):
    mix = pkg.SDMM(case["K"])
    mix.set_params(case["weights"], case["mean"], case["cov"])
    mix.set_state(case["state"])
    return mix


def _stats_dev(gpu, compact):
    import torch
    return torch.from_numpy(np.ascontiguousarray(compact, np.float64)).to(gpu)


def compare_step(oracle, K, p0, s0, p1, s1, stats_full, n_total, plog, tag):
    """One M-step of the GPU (p0, s0 -> p1, s1: get_params / get_state before
    and after) against or_mstep_f64 from the same p0, s0 and statistics, at
    the bounds of the module docstring.  Returns the realised figures."""
    band, (rc, po, so) = mc.reference_band(oracle, K, p0, s0, stats_full, n_total)
    assert band["stable"], "the inputs leave a decision to the last bits of eta (fix the inputs)"
    it = int(s0["scalars"][mc.IT])
    g = mc.gpu_state_named(s1)
    assert g["status"] == float(rc)
    assert g["it"] == so["it"]
    out = {"rc": rc, "state": {}, "off": 0, "off2": 0}
    # the step's own settings and the priors are inputs only
    np.testing.assert_array_equal(_bits(s1["scalars"][mc.ALPHA:mc.STATUS].copy()),
                                  _bits(s0["scalars"][mc.ALPHA:mc.STATUS].copy()), err_msg="alpha, ni, decp, cutoff")
    for n in ("bpriors", "bdepth"):
        np.testing.assert_array_equal(_bits(s1[n]), _bits(s0[n]), err_msg=n)
    if rc == 0:
        return out
    # ---- exact
    np.testing.assert_array_equal(p1["weights"] == 0, po["weights"] == 0, err_msg="killed / dead set")
    np.testing.assert_array_equal(p1["valid"], po["valid"], err_msg="valid")
    for n in oracle.MIX_FIELDS:
        a, b = np.asarray(p1[n], np.float32), np.asarray(po[n], np.float32)
        nf = ~np.isfinite(b)
        np.testing.assert_array_equal(~np.isfinite(a), nf, err_msg=f"non-finite pattern of {n}")
        np.testing.assert_array_equal(_bits(a)[nf], _bits(b)[nf], err_msg=f"non-finite bits of {n}")
    # ---- the fp64 state
    for n in mc.STATE_F64:
        a, b = np.asarray(g[n], np.float64).reshape(-1), np.asarray(so[n], np.float64).reshape(-1)
        assert np.isfinite(a).all() and np.isfinite(b).all(), n
        d = mc.rel_dist(a, b)
        out["state"][n] = d
        plog(f"{tag}_state_{n}_dist", d, 4 * band[n], band=band[n], iteration=it)
        if it == 0:
            np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=f"state {n} (it == 0: bitwise)")
        else:
            assert d <= 4 * band[n], f"state {n}: {d:.3e} vs 4 x band {band[n]:.3e}"
    if it == 0:
        np.testing.assert_array_equal(_bits(p1["cov"]), _bits(po["cov"]), err_msg="cov (it == 0: bitwise)")
        np.testing.assert_array_equal(_bits(p1["mean"][:, :3].copy()), _bits(po["mean"][:, :3].copy()),
                                      err_msg="mean[:, :3] (it == 0: bitwise)")
    # ---- float outputs
    fields = {n: (p1[n], po[n]) for n in oracle.MIX_FIELDS if n not in ("mean", "to")}
    fields["mean_pos"] = (p1["mean"][:, :3], po["mean"][:, :3])
    fields["mean_dir"] = (p1["mean"][:, 3:6], po["mean"][:, 3:6])
    fields["to"] = (p1["to"], po["to"])
    fields["normalization"] = (np.float32([g["normalization"]]), np.float32([so["normalization"]]))
    total = 0
    for n, (a, b) in fields.items():
        u = mc.ulp_distance(a, b)
        lim = 2 if n in TWO_ULP else 1
        total += u.size
        out["off2" if n in TWO_ULP else "off"] += int((u > 0).sum())
        assert u.max() <= lim, f"{n}: {int(u.max())} float ulps from the oracle (limit {lim}), {int((u > lim).sum())} entries"
        if it == 0 and n == "normalization":
            assert u.max() == 0
    plog(f"{tag}_float_entries_off_by_an_ulp", out["off"], total, iteration=it)
    plog(f"{tag}_sincos_float_entries_off", out["off2"], total, iteration=it)
    # ---- components that were not set keep every derived array
    notset = (po["weights"] == 0) | (np.asarray(so["sgW"]) == 0)
    assert (np.asarray(g["sgW"]) == 0).tolist() == (np.asarray(so["sgW"]) == 0).tolist()
    for n in oracle.MIX_FIELDS:
        if n in ("weights", "cdf"):
            continue
        np.testing.assert_array_equal(_bits(np.asarray(p1[n])[notset].copy()), _bits(np.asarray(p0[n])[notset].copy()),
                                      err_msg=f"{n} of a component that was not set")
    # ---- cdf
    cdf = p1["cdf"]
    assert (np.diff(cdf) >= 0).all()
    assert _bits(cdf[-1:])[0] == _bits(po["cdf"][-1:])[0], (cdf[-1], po["cdf"][-1])
    out["kills"] = int(((po["weights"] == 0) & (p0["weights"] != 0)).sum())
    return out


STEP_IDS = ["it%d-cut%d-decp%d-%s" % (s[0], s[1], s[2], "on" if s[3] else "off") for s in mc.STEP_CASES]


# ---- A: one M-step from constructed statistics ------------------------------
@pytest.mark.parametrize("step", mc.STEP_CASES, ids=STEP_IDS)
@pytest.mark.parametrize("K", KS)
def test_mstep_constructed_matches_oracle(pkg, oracle, gpu, plog, K, step):
    """sdmm_mstep (mstep_spread_kernel: ceil(Kp / 64) workgroups, the elected
    finish) on the ten families at once, n_total = 1000, against or_mstep_f64.

    Realised on the MI355X over the 49 cases (plog mstepA_*): at it == 0 every
    state array bitwise; at it > 0 the distance to the oracle, of the array's
    largest entry, is at most T 1.8e-16, sgW 2.2e-16, sgM 1.5e-16, sgC 3.3e-16,
    heuristicTotalWeight 0, sgH 0 -- at most 0.5 % of the measured band
    (3e-14 .. 4e-13); float entries that differ from the oracle at all: 0 of
    902727 (0 behind sin / cos)."""
    it, cutoff, decp, priors = step
    case = mc.build_case(K, it, priors=priors, decrease_prior=bool(decp), cutoff=cutoff)
    mix = _load(pkg, case)
    p0, s0 = mix.get_params(), mix.get_state()
    np.testing.assert_array_equal(s0["sgC"], case["state"]["sgC"])
    mix.mstep(_stats_dev(gpu, case["stats"]), case["n_total"])
    p1, s1 = mix.get_params(), mix.get_state()
    r = compare_step(oracle, K, p0, s0, p1, s1, case["stats_full"], case["n_total"], plog, "mstepA")
    assert r["rc"] == 1
    print(f"A K={K} {step}: kills {r['kills']} state dist {r['state']} floats off {r['off']} sincos off {r['off2']}")
    # the families did what they were built for, on the device
    po = mc.members(case, "pi_over")
    assert (p1["mean"][po] == 0).all() and (p1["weights"][po] > 0).all()
    if (not priors) or it == 40:
        assert (p1["weights"][mc.members(case, "indef")] == 0).all()
    if not priors:
        ns = mc.members(case, "nearsing")
        if ns.size >= len(mc.NEARSING_LAM):
            assert (p1["weights"][ns] == 0).any() and (p1["weights"][ns] > 0).any()
    mix.close()


def test_mstep_rejects_negative_n_total(pkg, gpu):
    """n_total < 0 is the sharded path's marker (the count rides behind the
    statistics, one element past sdmm_stats_len(K)); the public entry point
    refuses it and changes nothing."""
    case = mc.build_case(15, 3)
    mix = _load(pkg, case)
    p0, s0 = mix.get_params(), mix.get_state()
    st = _stats_dev(gpu, case["stats"])
    rc = pkg.lib().sdmm_mstep(mix.h, C.c_void_p(st.data_ptr()), C.c_int64(-1))
    assert rc == -1, rc                     # SDMM_E_INVALID
    with pytest.raises(pkg.SDMMError):
        mix.mstep(st, -5)
    p1, s1 = mix.get_params(), mix.get_state()
    for n, v in p0.items():
        np.testing.assert_array_equal(p1[n], v, err_msg=n)
    for n, v in s0.items():
        np.testing.assert_array_equal(s1[n], v, err_msg=n)
    mix.close()


# ---- B: sequences on one handle ---------------------------------------------
@pytest.mark.parametrize("K", [200, 512])
def test_mstep_sequence_on_one_handle(pkg, oracle, gpu, plog, K):
    """normal, zero_sum, normal, all_killed, normal on ONE handle, each
    mirrored on the oracle from the handle's own floats before it: an election
    counter that did not re-arm, or scratch (newW, vnew, dinew) left from an
    earlier launch, shows in the step after.  The zero_sum step changes
    nothing but STATUS (0); after all_killed every weight is 0 and stays 0.

    Realised on the MI355X: state distances at most 1.7e-16 (0.07 % of the
    band), 0 float entries differ."""
    case = mc.build_case(K, 3)
    killed = mc.all_killed_case(K, 3)
    mix = _load(pkg, case)
    normal = (_stats_dev(gpu, case["stats"]), case["stats_full"])
    zs = mc.zero_sum_stats(case)
    zero = (_stats_dev(gpu, zs), mc.full_stats(zs, K))
    allk = (_stats_dev(gpu, killed["stats"]), killed["stats_full"])
    for i, (name, (dev, full)) in enumerate([("normal", normal), ("zero_sum", zero), ("normal", normal),
                                             ("all_killed", allk), ("normal", normal)]):
        if name == "all_killed":
            # the all-indef state under the handle's own scalars, no priors
            st = mix.get_state()
            for n in ("T", "sgW", "sgM", "sgC", "bpriors", "bdepth"):
                st[n] = killed["state"][n]
            mix.set_state(st)
        p0, s0 = mix.get_params(), mix.get_state()
        mix.mstep(dev, case["n_total"])
        p1, s1 = mix.get_params(), mix.get_state()
        r = compare_step(oracle, K, p0, s0, p1, s1, full, case["n_total"], plog, f"mstepB{i}_{name}")
        print(f"B K={K} step {i} {name}: rc {r['rc']} state dist {r['state']} floats off {r['off']}")
        if name == "zero_sum":
            assert r["rc"] == 0 and s1["scalars"][mc.STATUS] == 0.0
            for n, v in p0.items():
                np.testing.assert_array_equal(_bits(np.asarray(p1[n], np.float32)) if n != "valid" else p1[n],
                                              _bits(np.asarray(v, np.float32)) if n != "valid" else v, err_msg=n)
            for n, v in s0.items():
                a, b = np.array(s1[n]), np.array(v)
                if n == "scalars":
                    a[mc.STATUS] = b[mc.STATUS] = 0.0
                np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=n)
        else:
            assert r["rc"] == 1 and s1["scalars"][mc.STATUS] == 1.0
        if i >= 3:
            assert (p1["weights"] == 0).all()
        if name == "all_killed":
            assert (p1["cdf"] == 0).all()
    assert int(mix.get_state()["scalars"][mc.IT]) == 3 + 4
    mix.close()


# ---- C: the batched form reaches the same branches ---------------------------
C_FAMILIES = ("dead", "pi_over", "tiny", "indef", "weak")


def state_driven_case(K, x, seed):
    """mstep_batched_kernel takes no statistics through the ABI, so the
    families come from the STATE: at it = 3 the blend keeps (1 - eta) of sgW,
    sgM, sgC.  pi_over, tiny, indef and weak components sit 40 units outside
    the sample box (their responsibilities underflow: statistics exactly 0,
    asserted by the test on the statistics themselves), so sgM / sgW and sgC
    are their blended mean and covariance; ord and dead ones sit on sample
    positions and directions with broad covariances.  No priors."""
    rng = np.random.default_rng([77, seed, K])
    fam = mc.family_of(K)
    keep = np.isin(fam, [mc.FAM[n] for n in C_FAMILIES])
    fam = np.where(keep, fam, mc.FAM["ord"])
    is_ = lambda *names: np.isin(fam, [mc.FAM[n] for n in names])
    far = is_("pi_over", "tiny", "indef", "weak")
    member = np.zeros(K, int)
    for f in range(10):
        idx = np.flatnonzero(fam == f)
        member[idx] = np.arange(idx.size)
    src = rng.choice(x.shape[1], K)
    pos = x[0:3, src].T.astype(np.float64)
    pos[far] += 40.0
    d = x[3:6, src].T.astype(np.float64)
    mean0 = np.concatenate([pos, d / np.linalg.norm(d, axis=1, keepdims=True)], 1)
    cov0 = np.tile(np.diag([0.05, 0.05, 0.05, 0.3, 0.3]), (K, 1, 1))
    w0 = rng.uniform(0.5, 1.5, K)
    w0[is_("dead")] = 0.0
    w0 /= w0.sum()
    length = rng.uniform(0.0, 0.3, K)
    for k in np.flatnonzero(is_("pi_over")):
        length[k] = mc.PI_OVER_LEN[member[k] % 2]
    for k in np.flatnonzero(is_("tiny")):
        length[k] = mc.TINY_LEN[member[k] % 5]
    phi = rng.uniform(0.0, 2.0 * np.pi, K)
    mu = np.concatenate([pos + rng.uniform(-0.05, 0.05, (K, 3)), (length * np.cos(phi))[:, None],
                         (length * np.sin(phi))[:, None]], 1)
    mu[is_("indef")] = 0.0
    S = np.stack([mc._spd(rng) for _ in range(K)])
    for k in np.flatnonzero(is_("indef")):
        q = mc._rot(rng, 5)
        S[k] = mc._sym(q @ np.diag(mc.INDEF_EIG) @ q.T)
    sgW = rng.uniform(0.5, 2.0, K)
    sgM = sgW[:, None] * mu
    sgC = mc._sym(sgW[:, None, None] * (S + mu[:, :, None] * mu[:, None, :]))
    wk = is_("weak")
    sgW[wk] = 0.0
    sgM[wk] = rng.uniform(-0.1, 0.1, (int(wk.sum()), 5))
    scalars = np.zeros(9)
    scalars[mc.HTW] = 1.1 * sgW.sum()
    scalars[mc.SGH] = 0.1 * sgW.sum()
    scalars[mc.NORM] = float(np.float32(0.7))
    scalars[mc.IT] = 3.0
    scalars[mc.ALPHA] = float(np.float32(0.9))
    scalars[mc.NI] = float(np.float32(6e-5))
    scalars[mc.DECP] = 1.0
    scalars[mc.CUT] = 32.0
    scalars[mc.STATUS] = 1.0
    state = {"scalars": scalars, "T": rng.uniform(0.5, 1.5, K) * scalars[mc.HTW], "sgW": sgW,
             "sgM": sgM.reshape(-1).copy(), "sgC": sgC.reshape(-1).copy(),
             "bpriors": np.zeros(25 * K, np.float32), "bdepth": np.zeros(9 * K, np.float32)}
    return {"K": K, "family": fam, "far": far, "weights": w0.astype(np.float32), "mean": mean0.astype(np.float32),
            "cov": cov0.astype(np.float32), "state": state}


@pytest.mark.parametrize("K", [72, 200])
def test_batched_mstep_reaches_the_branches(pkg, oracle, synth, gpu, plog, K):
    """One em_step_batched over n = 3 mixtures of a create_many table against
    three em_step on single handles holding the same parameters and state
    (state_driven_case), N = 257 samples each: every array of get_params() and
    get_state() bitwise equal; then the single handle's step against
    or_mstep_f64 fed the statistics of a clone taken before the step, at the
    bounds of compare_step.

    Realised on the MI355X: every state array bitwise the oracle's (distance
    0 at it = 3), 0 of 99558 float entries differ."""
    import torch
    N, n = 257, 3
    b = synth.em_batch(N * n, 128, guards=False)
    x, w = b["x"], b["w"]
    seg = np.arange(n + 1, dtype=np.int64) * N
    cases = [state_driven_case(K, x[:, seg[j]:seg[j + 1]], j) for j in range(n)]
    stream = torch.cuda.current_stream(gpu)
    hs = (C.c_void_p * n)()
    rc = pkg.lib().sdmm_create_many_on_stream(K, None, gpu.index, C.c_void_p(stream.cuda_stream), n, hs)
    assert rc == 0
    table = [pkg.SDMM._adopt(C.c_void_p(v), stream) for v in hs]
    single = [pkg.SDMM(K) for _ in range(n)]
    for grp in (table, single):
        for m, cs in zip(grp, cases):
            m.set_params(cs["weights"], cs["mean"], cs["cov"])
            m.set_state(cs["state"])
    clones = [m.clone() for m in single]
    ds = pkg.DeviceSamples.from_numpy(x, w)
    pkg.em_step_batched(table, ds, seg, 1)
    for j, m in enumerate(single):
        a, e = int(seg[j]), int(seg[j + 1])
        m.optimize(pkg.DeviceSamples([t[a:e] for t in ds.x], ds.w[a:e]), 1)
    torch.cuda.synchronize()
    for j in range(n):
        pb, ps = table[j].get_params(), single[j].get_params()
        for name in ps:
            np.testing.assert_array_equal(pb[name], ps[name], err_msg=f"mixture {j} {name}")
        sb, ss = table[j].get_state(), single[j].get_state()
        for name in ss:
            np.testing.assert_array_equal(_bits(sb[name]), _bits(ss[name]), err_msg=f"mixture {j} state {name}")
    for j in range(n):
        a, e = int(seg[j]), int(seg[j + 1])
        st = torch.zeros(pkg.stats_len(K), dtype=torch.float64, device=gpu)
        clones[j].estep_stats(pkg.DeviceSamples([t[a:e] for t in ds.x], ds.w[a:e]), st)
        clones[j].synchronize()
        compact = st.cpu().numpy()
        far = np.flatnonzero(cases[j]["far"])
        dead = mc.members(cases[j], "dead")
        # the check that the far (and the dead) components took no sample: their statistics are exactly 0
        for idx in (far, dead):
            assert (compact[2 + idx] == 0).all()
            assert (compact[2 + K:2 + 6 * K].reshape(K, 5)[idx] == 0).all()
            assert (compact[2 + 6 * K:].reshape(K, 15)[idx] == 0).all()
        assert compact[1] > 0 and (compact[2:2 + K] > 0).sum() >= K // 4
        p0, s0 = clones[j].get_params(), clones[j].get_state()
        p1, s1 = single[j].get_params(), single[j].get_state()
        r = compare_step(oracle, K, p0, s0, p1, s1, mc.full_stats(compact, K), N, plog, f"mstepC{j}")
        print(f"C K={K} mixture {j}: kills {r['kills']} state dist {r['state']} floats off {r['off']}")
        assert r["rc"] == 1
        cs = cases[j]
        po = mc.members(cs, "pi_over")
        assert (p1["mean"][po] == 0).all() and (p1["weights"][po] > 0).all()
        assert (p1["weights"][mc.members(cs, "indef")] == 0).all()
        assert (p1["weights"][dead] == 0).all()
        wk = mc.members(cs, "weak")
        assert (p1["weights"][wk] > 0).all() and np.ptp(p1["weights"][wk]) == 0
        np.testing.assert_array_equal(p1["cov"][wk], p0["cov"][wk])
    for m in table + single + clones:
        m.close()


# ---- D: set_params (MVTN::set alone) on edge components ----------------------
D_KINDS = 10


def set_edge_components(K):
    """(weights, means (K, 6), covs (K, 5, 5)) float32, kind k % D_KINDS:
    0 ordinary; 1 zero direction; 2 direction +z; 3 direction -z
    (coordinates_d divides by sign + n[2] = -2); 4 n[2] = -0.0 with a unit xy
    part; 5 (0, 0, -0.0); 6 5x5 not PD with a PD 3x3 block; 7 3x3 PD with a
    Schur complement that is not PD; 8 entries near 1e-30; 9 near 1e30."""
    rng = np.random.default_rng([5, K])
    w = rng.uniform(0.5, 1.5, K)
    mean = np.concatenate([rng.uniform(0.2, 0.8, (K, 3)), mc._unit(rng.normal(size=(K, 3)))], 1)
    cov = np.stack([mc._spd(rng) for _ in range(K)])
    kind = np.arange(K) % D_KINDS
    for k in range(K):
        if kind[k] == 1:
            mean[k, 3:] = 0.0
        elif kind[k] == 2:
            mean[k, 3:] = (0.0, 0.0, 1.0)
        elif kind[k] == 3:
            mean[k, 3:] = (0.0, 0.0, -1.0)
        elif kind[k] == 4:
            mean[k, 3:] = (0.6, 0.8, -0.0) if (k // D_KINDS) % 2 else (1.0, 0.0, -0.0)
        elif kind[k] == 5:
            mean[k, 3:] = (0.0, 0.0, -0.0)
        elif kind[k] == 6:
            # PD position block, a directional block far too small for the coupling
            c = np.diag([0.04, 0.05, 0.06, 0.01, 0.02])
            c[0, 3] = c[3, 0] = 0.05
            cov[k] = c
        elif kind[k] == 7:
            c = np.diag([0.04, 0.05, 0.06, 0.02, 0.03])
            c[1, 4] = c[4, 1] = 0.06      # S[1, 1] = 0.03 - 0.06^2 / 0.05 < 0
            cov[k] = c
        elif kind[k] == 8:
            cov[k] *= 1e-28               # entries 1e-31 .. 1e-29
        elif kind[k] == 9:
            cov[k] *= 1e31                # entries 1e28 .. 1e30
    return w / w.sum(), mean.astype(np.float32), cov.astype(np.float32), kind


@pytest.mark.parametrize("K", [15, 512])
def test_set_params_edge_components(pkg, oracle, gpu, plog, K):
    """set_all_kernel (one workgroup) against oracle.Mixture.set_component(mode=1)
    + configure(), both from the same prior arrays (an ordinary mixture set
    first), so that what a failed factorisation must leave alone can be
    checked: every field within 1 float ulp (non-finite bits exact), valid exact.

    Realised on the MI355X: 0 entries differ at K = 15 and K = 512."""
    base = mc.build_case(K, 0)
    mix = pkg.SDMM(K)
    mix.set_params(base["weights"], base["mean"], base["cov"])
    prior = mix.get_params()
    assert (prior["valid"] == 1).all()
    w, mean, cov, kind = set_edge_components(K)
    mix.set_params(w, mean, cov)
    p = mix.get_params()
    m = oracle.Mixture(K)
    m.copy_params_from(prior)
    m.valid[:] = prior["valid"]
    m.weights[:] = w.astype(np.float32)
    for k in range(K):
        m.set_component(k, mean[k].astype(np.float64), cov[k].astype(np.float64), mode=1)
    m.configure()
    np.testing.assert_array_equal(p["valid"], m.valid)
    off = 0
    for n in oracle.MIX_FIELDS:
        a, r = np.asarray(p[n], np.float32), np.asarray(getattr(m, n), np.float32)
        nf = ~np.isfinite(r)
        np.testing.assert_array_equal(_bits(a)[nf], _bits(r)[nf], err_msg=f"non-finite bits of {n}")
        u = mc.ulp_distance(a, r)
        off += int((u > 0).sum())
        assert u.max() <= 1, f"{n}: {int(u.max())} float ulps, kinds {np.unique(kind[np.flatnonzero(u.reshape(K, -1).max(1) > 1)])}"
    plog(f"set_params_edges_K{K}_float_entries_off_by_an_ulp", off, 0)
    print(f"D K={K}: float entries off by an ulp: {off}")
    k6, k7 = np.flatnonzero(kind == 6), np.flatnonzero(kind == 7)
    assert (p["valid"][k6] == 0).all() and (p["valid"][k7] == 0).all()
    assert (p["valid"][~np.isin(kind, (6, 7))] == 1).all()
    for n in ("cholL", "cholLInv", "detInv"):          # the failed 5x5 factorisation leaves them
        np.testing.assert_array_equal(_bits(p[n][k6].copy()), _bits(prior[n][k6].copy()), err_msg=n)
        np.testing.assert_array_equal(_bits(p[n][k7].copy()), _bits(prior[n][k7].copy()), err_msg=n)
    assert (_bits(p["margL"][k6].copy()) != _bits(prior["margL"][k6].copy())).any(1).all()   # margL is set
    np.testing.assert_allclose(p["margL"][k6][:, 0], np.sqrt(cov[k6][:, 0, 0].astype(np.float64)), rtol=1e-6)
    for n in ("condL", "condLInv", "condDetInv"):      # the failed Schur factorisation leaves them
        np.testing.assert_array_equal(_bits(p[n][k7].copy()), _bits(prior[n][k7].copy()), err_msg=n)
    # -z: the frame is finite and orthonormal
    k3 = np.flatnonzero(kind == 3)
    to = p["to"][k3].reshape(-1, 3, 3).astype(np.float64)
    np.testing.assert_allclose(to @ to.transpose(0, 2, 1), np.tile(np.eye(3), (k3.size, 1, 1)), atol=1e-6)
    mix.close()


# ---- E: the packed records the kernels read ----------------------------------
def samples_from_mixture(p, N, seed=3):
    """N samples at the live, valid components of p that have a direction:
    position mean + 0.5 cholL z, direction the mean's moved by half a
    directional standard deviation."""
    rng = np.random.default_rng(seed)
    ok = np.flatnonzero((p["weights"] > 0) & (p["valid"] == 1) & (np.abs(p["mean"][:, 3:6]).sum(1) > 0))
    k = ok[np.arange(N) % ok.size]
    L = p["cholL"].reshape(-1, 5, 5)[k][:, :3, :3].astype(np.float64)
    pos = p["mean"][k, :3] + 0.5 * np.einsum("nij,nj->ni", L, rng.normal(size=(N, 3)))
    sd = np.sqrt(p["cov"].reshape(-1, 5, 5)[k, 3, 3].astype(np.float64))
    d = mc._unit(p["mean"][k, 3:6] + 0.5 * sd[:, None] * rng.normal(size=(N, 3)))
    return np.concatenate([pos, d], 1).T.astype(np.float32).copy()


def test_packed_records_after_mstep(pkg, oracle, synth, gpu, plog):
    """After the K = 200, it = 3 step of A: posterior on N = 257 samples and
    guide on 257 queries read the packed records, whose weight fields (EP_PI,
    EP_DIPI, GP_W) the finishing wave wrote from vnew / dinew.  Columns of
    zero-weight or invalid components exactly 0; the rest at the bound of
    test_gpu_parity._check_resp; guide indices bit-exact."""
    import torch
    from test_gpu_parity import _check_resp
    K, N = 200, 257
    case = mc.build_case(K, 3)
    # three ordinary components start INVALID (a 5x5 that is not positive
    # definite over a PD 3x3 block) and the step makes them valid: the weight
    # fields must come from the flag the blend publishes (vnew), not the old one
    flip = mc.members(case, "ord")[:3]
    bad = np.diag([0.04, 0.05, 0.06, 0.01, 0.02])
    bad[0, 3] = bad[3, 0] = 0.05
    case["cov"][flip] = bad.astype(np.float32)
    mix = _load(pkg, case)
    before = mix.get_params()
    assert (before["valid"][flip] == 0).all() and before["valid"].sum() == K - 3
    mix.mstep(_stats_dev(gpu, case["stats"]), case["n_total"])
    p = mix.get_params()
    assert (p["valid"][flip] == 1).all() and (p["weights"][flip] > 0).all()
    om = oracle.Mixture(K)
    om.copy_params_from(p)
    om.valid[:] = p["valid"]
    x = samples_from_mixture(p, N)
    w = np.ones(N, np.float32)
    ds = pkg.DeviceSamples.from_numpy(x, w)
    resp = torch.full((N, K), -1.0, device=gpu)
    mix.posterior(ds, resp)
    torch.cuda.synchronize()
    got = resp.cpu().numpy()
    off = (p["weights"] == 0) | (p["valid"] == 0)
    assert off.any() and (got[:, off] == 0).all()
    ref = oracle.responsibilities(om, oracle.Samples(x, w))
    assert (ref[:, p["weights"] == 0] == 0).all()
    live = dict(p)                          # the fp64 side knows no valid flag: an invalid component has pi = 0
    live["weights"] = np.where(p["valid"] == 1, p["weights"], np.float32(0.0))
    _check_resp(got, ref, live, x, plog)
    assert (got[:, flip].max(0) > 1e-3).all(), "a component that became valid has no posterior mass"
    c = x[0:3].copy()
    _, u = synth.queries(N)
    ct = [torch.from_numpy(c[i].copy()).to(gpu) for i in range(3)]
    ut = [torch.from_numpy(u[i].copy()).to(gpu) for i in range(3)]
    d, pdf, comp = mix.guide(ct, ut)
    torch.cuda.synchronize()
    dr, pr, cr, _ = oracle.guide_batch(om, c.T, u.T)
    plog("mstepE_guide_index_mismatches", int((comp.cpu().numpy() != cr).sum()), 0)
    np.testing.assert_array_equal(comp.cpu().numpy(), cr)
    assert (cr >= 0).sum() > N // 2 and not off[cr[cr >= 0]].any()
    mix.close()
