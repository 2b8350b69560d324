"""The band form of the split responsibility kernel at K = 128.

estep_resp_split_band_kernel (estep_split.hip) keeps the coefficient image in
registers: wave w of a 4-wave workgroup owns components 32 w .. 32 w + 31, the
work unit is a super-tile of 64 samples (wave w builds and stores tile w), the
super-tiles are dealt round robin over one round of resident workgroups, and
the posterior normaliser is the sum of the four waves' partials.  Checked here:

  * the edges of the deal: fewer samples than a tile, than a super-tile, one
    more, a launch just above two rounds of resident workgroups with a 7-row
    tail.  resp is pre-filled with -1 and has guard rows: every row below n is
    written, nothing beyond it, and the values hold the bound of
    test_gpu_parity._check_resp against the oracle;
  * old versus new: against a handle of the same parameters created under
    SDMM_RESP_KERNEL=splitlds (the coefficient image in LDS, every sample's 128
    components summed in one wave) the unnormalised pdfs are the same bits and
    only the normaliser's summation order differs: 128 non-negative terms, any
    order within 127 2^-24 relative, v_rcp a couple of ulps more, so
    |new - old| <= 2^-16 old + 2^-126 per entry, and exact zeros agree; at
    K = 128, 100, 72 (K < Kp: the partial store path), with and without the
    optional planes;
  * placement invariance: posterior(batch)[a:b] equals posterior(batch[a:b])
    bit for bit;
  * quirk inputs: a rare angle, a NaN feature and a zero direction in each of
    the four tiles of a super-tile, the rare component in each wave's band and
    in both of its blocks.

Every batch but the "no planes" one carries both optional planes (hpdf and the
isDiffuse bytes, half of them set).
"""
import numpy as np
import pytest

from test_gpu_parity import _check_resp

pytestmark = pytest.mark.gpu

GUARD_ROWS = 5
REL, ABS = 2.0 ** -16, 2.0 ** -126
_cache = {}


def _mixture(pkg, synth, b, K):
    """The first K components of the hemisphere initialisation of the next
    multiple of 8, weights renormalised (the same parameters for every handle)."""
    pos, nrm = synth.model_seed_points(b, 8 * ((K + 7) // 8))
    h = pkg.hemisphere_init_host(pos, nrm, synth.DEPTH_PRIOR, synth.SPATIAL_DISTANCE, synth.SEED_MODEL)
    mix = pkg.SDMM(K)
    mix.set_params(h["weights"][:K] / h["weights"][:K].sum(), h["mean"][:K], h["cov"][:K])
    return mix


def _case(pkg, synth, K, N, monkeypatch=None):
    """One seeded batch and the band handle per (K, N); with monkeypatch also
    the splitlds twin of the same parameters."""
    key = (K, N)
    if key not in _cache:
        b = synth.em_batch(N, 128, heuristic=True)
        mix = _mixture(pkg, synth, b, K)
        name = mix.kernel_name("resp")
        assert "split_band" in name, name
        ds = pkg.DeviceSamples.from_numpy(b["x"], b["w"], b["hpdf"], b["is_diffuse"])
        _cache[key] = {"b": b, "mix": mix, "ds": ds, "lds": None, "om": None}
    c = _cache[key]
    if monkeypatch is not None and c["lds"] is None:
        monkeypatch.setenv("SDMM_RESP_KERNEL", "splitlds")
        c["lds"] = _mixture(pkg, synth, c["b"], K)
        name = c["lds"].kernel_name("resp")
        assert "split" in name and "band" not in name, name
        monkeypatch.delenv("SDMM_RESP_KERNEL")
    return c


def _oracle_rows(c, oracle, rows):
    """The fp32 oracle's responsibilities of the given rows, from the device's
    derived parameters."""
    if c["om"] is None:
        p = c["mix"].get_params()
        c["om"] = oracle.Mixture(p["weights"].shape[0])
        c["om"].copy_params_from(p)
        c["om"].valid[:] = p["valid"]
    b = c["b"]
    return oracle.responsibilities(c["om"], oracle.Samples(b["x"][:, rows], b["w"][rows], b["hpdf"][rows],
                                                           b["is_diffuse"][rows]))


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


def _check_rows(c, got, ref, rows, min_frac=0.5):
    b = c["b"]
    _check_resp(got, ref, c["mix"].get_params(), b["x"][:, rows], None, b["hpdf"][rows], b["is_diffuse"][rows],
                min_frac=min_frac)


def _within_bound(new, old, what):
    """|new - old| <= 2^-16 old + 2^-126 per entry, exact zeros agree."""
    new64, old64 = new.astype(np.float64), old.astype(np.float64)
    excess = np.abs(new64 - old64) - (REL * old64 + ABS)
    worst = np.unravel_index(np.argmax(excess), excess.shape)
    nz = old64 > 2.0 ** -100
    rel = float((np.abs(new64 - old64)[nz] / old64[nz]).max(initial=0.0))
    print(f"{what}: max relative difference {rel:.3e} (bound {REL:.3e})")
    assert excess.max() <= 0.0, f"{what}: entry {worst}: new {new[worst]!r} old {old[worst]!r}"
    zeros = (new == 0) != (old == 0)
    assert not zeros.any(), f"{what}: {int(zeros.sum())} entries are zero in one build only, first {np.argwhere(zeros)[:4]}"


N_SMALL = 4 * 64 + 1


@pytest.mark.parametrize("n", [1, 16, 63, 64, 65, N_SMALL])
def test_deal_small_launches(pkg, oracle, synth, gpu, n):
    """Fewer super-tiles than resident workgroups: waves whose tile lies past n
    still run the super-tile's barriers and pair math, and store nothing."""
    K = 128
    c = _case(pkg, synth, K, N_SMALL)
    if "ref" not in c:
        c["ref"] = _oracle_rows(c, oracle, np.arange(N_SMALL))
    got = _posterior(c["mix"], _slice(pkg, c["ds"], 0, n), K, gpu)
    # (the explained-share guard of _check_resp is a statistic of many rows)
    _check_rows(c, got, c["ref"][:n], np.arange(n), min_frac=0.5 if n >= 64 else 0.0)


def _big_n(gpu):
    import torch
    G = 3 * torch.cuda.get_device_properties(gpu).multi_processor_count   # resident 4-wave workgroups
    return 64 * (2 * G + G // 3 + 5) + 7, G


def test_deal_just_above_two_rounds(pkg, oracle, synth, gpu):
    """n = 64 (2 G + G / 3 + 5) + 7 with G resident workgroups: a third of them
    serve three super-tiles, the rest two; the last super-tile has 7 rows, all
    in wave 0's tile."""
    K = 128
    n, G = _big_n(gpu)
    c = _case(pkg, synth, K, n)
    got = _posterior(c["mix"], c["ds"], K, gpu)
    c["full"] = got
    # the CPU side on a few hundred rows: the first and last super-tiles, both
    # ends of every round of workgroups, and a seeded sample of the rest
    edges = [0, 64 * G, 128 * G, 64 * (2 * G + G // 3), n - 23]
    rows = np.concatenate([np.arange(max(e - 16, 0), min(e + 32, n)) for e in edges]
                          + [np.random.default_rng(0xBA2D).choice(n, size=256, replace=False)])
    rows = np.unique(rows)
    _check_rows(c, got[rows], _oracle_rows(c, oracle, rows), rows)


@pytest.mark.parametrize("a", [1, 2, 3, 21])
def test_placement_invariance_bitwise(pkg, oracle, synth, gpu, a):
    """posterior(batch)[a:b] == posterior(batch[a:b]), bit for bit: the slice
    moves every sample to another workgroup, tile and lane and, for a not a
    multiple of 4, the flag bytes to another place in their dwords."""
    K = 128
    n, G = _big_n(gpu)
    c = _case(pkg, synth, K, n)
    if "full" not in c:
        c["full"] = _posterior(c["mix"], c["ds"], K, gpu)
    b = n - 30 - a
    assert (b - a) % 16 != 0
    part = _posterior(c["mix"], _slice(pkg, c["ds"], a, b), K, gpu)
    diff = np.flatnonzero((part != c["full"][a:b]).any(1))
    assert np.array_equal(part, c["full"][a:b]), f"{diff.size} rows differ, first at slice rows {diff[:8]}"


@pytest.mark.parametrize("planes", [True, False])
@pytest.mark.parametrize("K", [128, 100, 72])
def test_band_equals_lds_image_kernel(pkg, synth, gpu, monkeypatch, K, planes):
    """Old versus new on one mixture, n = 1000 (K < Kp = 128: every row through
    the partial store path; planes False: hpdf = None, is_diffuse = None)."""
    n = 1000
    c = _case(pkg, synth, K, n, monkeypatch)
    ds = c["ds"] if planes else pkg.DeviceSamples(list(c["ds"].x), c["ds"].w)
    if planes:
        new, old = _posterior(c["mix"], ds, K, gpu), _posterior(c["lds"], ds, K, gpu)
    else:
        import torch
        out = []
        for mix in (c["mix"], c["lds"]):
            resp = torch.full((n + GUARD_ROWS, K), -1.0, device=gpu)
            mix.posterior(ds, resp)
            torch.cuda.synchronize()
            r = resp.cpu().numpy()
            assert (r[n:] == -1.0).all() and (r[:n] >= 0.0).all()
            out.append(r[:n])
        new, old = out
    assert (old.sum(1) > 0).mean() > 0.5
    _within_bound(new, old, f"K={K} planes={planes}")


def test_quirk_inputs_in_every_tile_and_band(pkg, synth, gpu, monkeypatch):
    """Eight super-tiles; in super-tile j, tile t holds a sample 7.5e-4 ..
    8.5e-4 rad from antipodal to component 16 j + 4 t + 3's mean direction at
    its spatial mean (the far-side quirk, c < -0.9999995: block j, i.e. wave
    j / 2's band and its block j % 2 -- that wave flags the tile and all four
    redo it), tile j % 4 a sample with a NaN feature and tile (j + 1) % 4 one
    with a zero direction."""
    import torch
    K, n = 128, 8 * 64
    c = _case(pkg, synth, K, n, monkeypatch)
    b = c["b"]
    mu = c["mix"].get_params()["mean"].astype(np.float64)
    x = b["x"].copy()
    rng = np.random.default_rng(19)
    rare, nan_rows, zero_rows = [], [], []
    for j in range(8):
        for t in range(4):
            i, k = 64 * j + 16 * t + 3 + t, 16 * j + 4 * t + 3
            d = mu[k, 3:6] / np.linalg.norm(mu[k, 3:6])
            tt = np.cross(d, [0.0, 0.0, 1.0] if abs(d[2]) < 0.9 else [1.0, 0.0, 0.0])
            tt /= np.linalg.norm(tt)
            dl = rng.uniform(7.5e-4, 8.5e-4)
            x[0:3, i] = mu[k, 0:3].astype(np.float32)
            x[3:6, i] = (-np.cos(dl) * d + np.sin(dl) * tt).astype(np.float32)
            rare.append((i, k))
        nan_rows.append(64 * j + 16 * (j % 4) + 9)
        zero_rows.append(64 * j + 16 * ((j + 1) % 4) + 12)
    x[1, nan_rows] = np.nan
    x[3:6, zero_rows] = 0.0
    xt = [torch.from_numpy(x[i].copy()).to(gpu) for i in range(6)]
    ds = pkg.DeviceSamples(xt, c["ds"].w, c["ds"].hpdf, c["ds"].is_diffuse)
    out = []
    for mix in (c["mix"], c["lds"]):
        resp = torch.full((n + GUARD_ROWS, K), -1.0, device=gpu)
        mix.posterior(ds, resp)
        torch.cuda.synchronize()
        r = resp.cpu().numpy()
        assert (r[n:] == -1.0).all() and np.isfinite(r[:n]).all() and (r[:n] >= 0.0).all()
        out.append(r[:n])
    new, old = out
    assert (new[nan_rows] == 0).all() and (new[zero_rows] == 0).all()
    assert (old[nan_rows] == 0).all() and (old[zero_rows] == 0).all()
    # the quirk is in play: the targeted component (jacobian 1 instead of the
    # angle over its vanishing sine) holds a visible share of its row
    share = np.array([old[i, k] for i, k in rare])
    assert np.median(share) > 0.01, share
    _within_bound(new, old, "quirk inputs")
