"""The split responsibility kernel's tile deal, tail and row addressing.

estep_resp_split_kernel (estep_split.hip) deals the launch's 16-sample tiles
round robin over one round of resident waves, numbered in quads across the
workgroups, and addresses its rows and its sample records from wave-uniform
bases that step with the tiles.  Checked here:

  * the edges of the deal: fewer samples than a tile, than a workgroup's waves,
    one more than that; a launch just above two full rounds of resident waves
    (waves differ by one tile, every wave runs its address stepping); K below
    the padded Kp and the R = 1, 2, 4 configurations (the partial and the
    unstaged flush).  resp is pre-filled with -1 and has guard rows: every row
    below n is written, nothing beyond it, and the values hold the bound of
    test_gpu_parity._check_resp against the oracle;
  * placement invariance: a sample's row does not depend on where the sample
    lies in the launch (which wave and tile serve it, how the planes are
    aligned) -- posterior(batch)[a:b] equals posterior(batch[a:b]) bit for bit.

Every batch carries both optional planes (hpdf and the isDiffuse bytes, half
of them set), so the flag byte's place in its dword is part of every check.
"""
import numpy as np
import pytest

from test_gpu_parity import _check_resp, _setup

pytestmark = pytest.mark.gpu

GUARD_ROWS = 5
WPB = 12          # waves per workgroup of the K = 128 configuration
_cache = {}


def _case(pkg, oracle, synth, K, N, with_ref=True):
    """One seeded batch, model and fp32-oracle reference per (K, N), shared."""
    key = (K, N)
    if key not in _cache:
        if K % 8 == 0:
            b, mix, om, ost, ds, os_ = _setup(pkg, oracle, synth, K, N, heuristic=True)
        else:
            # uniformHemisphereInit makes 8 components per seed point: the
            # first K of the next multiple's, weights renormalised, set as
            # parameters; the oracle takes the device's derived parameters
            b = synth.em_batch(N, 128, heuristic=True)
            pos, nrm = synth.model_seed_points(b, 8 * (K // 8 + 1))
            h = pkg.hemisphere_init_host(pos, nrm, synth.DEPTH_PRIOR, synth.SPATIAL_DISTANCE, synth.SEED_MODEL)
            mix = pkg.SDMM(K)
            mix.set_params(h["weights"][:K] / h["weights"][:K].sum(), h["mean"][:K], h["cov"][:K])
            p = mix.get_params()
            om = oracle.Mixture(K)
            om.copy_params_from(p)
            om.valid[:] = p["valid"]
            ds = pkg.DeviceSamples.from_numpy(b["x"], b["w"], b["hpdf"], b["is_diffuse"])
            os_ = oracle.Samples(b["x"], b["w"], b["hpdf"], b["is_diffuse"])
        assert "split" in mix.kernel_name("resp"), mix.kernel_name("resp")
        _cache[key] = {"b": b, "mix": mix, "om": om, "ds": ds, "os": os_, "ref": None}
    c = _cache[key]
    if with_ref and c["ref"] is None:
        c["ref"] = oracle.responsibilities(c["om"], c["os"])
    return c


def _slice(pkg, ds, a, b):
    return pkg.DeviceSamples([t[a:b] for t in ds.x], ds.w[a:b], ds.hpdf[a:b], ds.is_diffuse[a:b])


def _posterior(mix, ds, K, gpu):
    """Rows [0, n) of a -1-filled resp with guard rows; the guards stay -1 and
    no written row keeps a -1 (responsibilities are >= 0)."""
    import torch
    n = ds.n
    resp = torch.full((n + GUARD_ROWS, K), -1.0, device=gpu)
    mix.posterior(ds, resp)
    torch.cuda.synchronize()
    out = resp.cpu().numpy()
    assert (out[n:] == -1.0).all(), "rows beyond n were written"
    unwritten = np.flatnonzero((out[:n] == -1.0).any(1))
    assert unwritten.size == 0, f"rows never written: {unwritten[:8]} (of {unwritten.size})"
    assert np.isfinite(out[:n]).all()
    return out[:n]


def _check_rows(c, got, rows, min_frac=0.5):
    b = c["b"]
    _check_resp(got, c["ref"][rows], c["mix"].get_params(), b["x"][:, rows], None,
                b["hpdf"][rows], b["is_diffuse"][rows], min_frac=min_frac)


@pytest.mark.parametrize("n", [1, 15, 16, 17, 16 * WPB - 1, 16 * WPB + 1])
def test_deal_small_launches(pkg, oracle, synth, gpu, n):
    """Fewer tiles than resident waves: the launch has ceil(tiles / 12)
    workgroups, the waves beyond the tiles exit, the last tile is partial."""
    K = 128
    c = _case(pkg, oracle, synth, K, 16 * WPB + 1)
    got = _posterior(c["mix"], _slice(pkg, c["ds"], 0, n), K, gpu)
    # (the explained-share guard of _check_resp is a statistic of many rows)
    _check_rows(c, got, np.arange(n), min_frac=0.5 if n >= 64 else 0.0)


def _big_n(gpu):
    import torch
    W = WPB * torch.cuda.get_device_properties(gpu).multi_processor_count
    return 16 * (2 * W + W // 3 + 5) + 7, W


def test_deal_just_above_two_rounds(pkg, oracle, synth, gpu):
    """n = 16 (2 W + W / 3 + 5) + 7 with W resident waves: a third of the waves
    serve three tiles, the rest two, and the last tile has 7 rows."""
    K = 128
    n, W = _big_n(gpu)
    c = _case(pkg, oracle, synth, K, n, with_ref=False)
    got = _posterior(c["mix"], c["ds"], K, gpu)
    # the CPU side on a few hundred rows: the first and last tiles, both ends
    # of every round of waves, and a seeded sample of the rest
    edges = [0, 16 * W, 32 * W, 16 * (2 * W + W // 3), n - 23]
    rows = np.concatenate([np.arange(max(e - 16, 0), min(e + 32, n)) for e in edges]
                          + [np.random.default_rng(0xDEA1).choice(n, size=256, replace=False)])
    rows = np.unique(rows)
    b = c["b"]
    ref = oracle.responsibilities(c["om"], oracle.Samples(b["x"][:, rows], b["w"][rows], b["hpdf"][rows],
                                                          b["is_diffuse"][rows]))
    _check_resp(got[rows], ref, c["mix"].get_params(), b["x"][:, rows], None, b["hpdf"][rows],
                b["is_diffuse"][rows])


@pytest.mark.parametrize("K", [16, 32, 64, 100])
def test_deal_other_configurations(pkg, oracle, synth, gpu, monkeypatch, K):
    """R = 1, 2, 4 (full tiles stored without the LDS stage) and K = 100 < Kp =
    128 (every tile through the partial flush), five tiles and three rows."""
    monkeypatch.setenv("SDMM_RESP_KERNEL", "split")
    n = 16 * 4 * 5 + 3
    c = _case(pkg, oracle, synth, K, n)
    got = _posterior(c["mix"], c["ds"], K, gpu)
    _check_rows(c, got, np.arange(n))


@pytest.mark.parametrize("a", [1, 2, 3, 21])
def test_placement_invariance_bitwise(pkg, oracle, synth, gpu, a):
    """posterior(batch)[a:b] == posterior(batch[a:b]), bit for bit: the slice
    moves every sample to another wave and tile and, for a not a multiple of 4,
    the flag bytes to another place in their dwords."""
    K = 128
    n, W = _big_n(gpu)
    c = _case(pkg, oracle, synth, K, n, with_ref=False)
    if "full" not in c:
        c["full"] = _posterior(c["mix"], c["ds"], K, gpu)
    b = n - 30 - a                      # b - a = n - 30 - 2 a: checked below
    assert (b - a) % 16 != 0
    part = _posterior(c["mix"], _slice(pkg, c["ds"], a, b), K, gpu)
    diff = np.flatnonzero((part != c["full"][a:b]).any(1))
    assert np.array_equal(part, c["full"][a:b]), f"{diff.size} rows differ, first at slice rows {diff[:8]}"
