"""GPU: a learned BSDF over a C-dimensional condition conditioned on the device
(sdmm_learned_conditional_device; the learned_bsdf.h code the render's Phong
product bounces run in li_compact_kernel) -- BITWISE the host ABI
(sdmm_learned_conditional, pinned by tests/test_learned_nd.py): lobe counts,
weights, means and covariances, with per-query condition planes and with the
scalar broadcast, pruned / forced / unpruned, over incident directions on and
below the horizon and a ragged last block."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NQ = 4097          # 16 full blocks of 256 and one thread


def _directions(rng, nq):
    th = rng.uniform(0.0, 1.75, nq)                      # some below the horizon: no valid getDMM
    ph = rng.uniform(0.0, 2 * np.pi, nq)
    return np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)]).astype(np.float32)


def _compare(L, rest_of, W, out, keep, force, queries):
    w, mean, cov, n = (x.cpu().numpy() for x in out)
    rows = keep if keep > 0 else 8
    assert w.shape == (W.shape[1], rows)
    assert (n[W[2] <= 0] == 0).all() and (n[W[2] > 0] > 0).all()
    for q in queries:
        hw, hm, hc = L.conditional(rest_of(q), W[:, q], keep, force)
        k = len(hw)
        assert n[q] == k
        np.testing.assert_array_equal(w[q, :k], hw)
        np.testing.assert_array_equal(mean[q, :k], hm)
        np.testing.assert_array_equal(cov[q, :k], hc)
        assert (w[q, k:] == 0).all()
    return n


@pytest.mark.parametrize("keep", [0, 2, 3])
@pytest.mark.parametrize("force", [-1, 1])
def test_device_conditional_equals_host_bitwise(pkg, scenes, gpu, keep, force):
    import torch
    L = pkg.LearnedBSDFND.load_json(scenes.LEARNED_PHONG)
    rng = np.random.default_rng(100 + 10 * keep + force)
    W = _directions(rng, NQ)
    spec = rng.uniform(0.0, 1.0, NQ).astype(np.float32)
    lexp = np.log(np.exp(rng.uniform(0.0, np.log(1000.0), NQ))).astype(np.float32)   # exponents 1 .. 1000
    lexp[:2] = np.float32([0.0, np.log(1000.0)])
    Wt = [torch.from_numpy(W[i].copy()).to(gpu) for i in range(3)]
    queries = np.concatenate([[0, 1, NQ - 1], rng.choice(NQ, 497, replace=False)])
    # per-query planes
    out = L.conditional_device([torch.from_numpy(spec).to(gpu), torch.from_numpy(lexp).to(gpu)], Wt, keep, force)
    torch.cuda.synchronize()
    n = _compare(L, lambda q: [spec[q], lexp[q]], W, out, keep, force, queries)
    up = W[2] > 0
    assert (n[up] == (keep if keep else 4)).all()        # the shipped model covers every condition
    # one plane, one broadcast scalar; then both broadcast
    out = L.conditional_device([0.4, torch.from_numpy(lexp).to(gpu)], Wt, keep, force)
    torch.cuda.synchronize()
    _compare(L, lambda q: [np.float32(0.4), lexp[q]], W, out, keep, force, queries)
    out = L.conditional_device([0.4, float(np.log(30.0))], Wt, keep, force)
    torch.cuda.synchronize()
    _compare(L, lambda q: [np.float32(0.4), np.float32(np.log(30.0))], W, out, keep, force, queries)


def test_device_conditional_c2_equals_sdmm4_kernel(pkg, scenes, gpu):
    """C = 2 through the new kernel == the SDMM4 kernel, bitwise, with alpha as
    a plane (constant here) and as the scalar."""
    import torch
    m = scenes.load_learned()
    L4, L = pkg.LearnedBSDF(*m), pkg.LearnedBSDFND(*m)
    W = _directions(np.random.default_rng(9), NQ)
    Wt = [torch.from_numpy(W[i].copy()).to(gpu) for i in range(3)]
    ref = L4.conditional_device(0.2, Wt, 2)
    plane = torch.full((NQ,), 0.2, device=gpu)
    for rest in ([0.2], [plane]):
        out = L.conditional_device(rest, Wt, 2, -1)
        torch.cuda.synchronize()
        assert torch.equal(out[3], ref[3])
        live = (ref[3] > 0)
        for a, b in zip(out[:3], ref[:3]):
            assert torch.equal(a[live], b[live])
