"""CPU: the oracle's rough dielectric (oracle/sdmm_oracle_li.inc:
li_roughdielectric_sample / _eval_pdf / _crossed, kind 4 in li_path) -- the
restatement the device Li is compared with in
tests/test_gpu_li_oracle_dielectric.py -- shown right on its own:

  * bit for bit equal to the library's host call (csrc/bsdf_roughdielectric.h
    through sdmm_bsdf_roughdielectric_host; both run here with the same C
    library, so a difference is one of code) on the batch test's edge rows;
  * against roughdielectric.cpp in float64 with the host test's tolerances and
    exemptions (test_bsdf_roughdielectric.check_matches_float64);
  * the oracle's Li on a free-standing pane against the float64 albedo -- a
    check that does not go through the library at all;
  * threads do not change results; the product conditional of kind 4 is the
    library's."""
import numpy as np
import pytest

from test_bsdf_roughdielectric import ETA, HostBsdf, check_matches_float64, sphere_wi
from test_gpu_roughdielectric import SE_MIN, _furnace, _known_answer, edge_rows

LEAF = (np.float32([[0, 0, 0, 1, 1, 1]]), np.int32([[-1, -1]]))      # a one-node tree: unguided renders


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


class OracleBsdf:
    """or_bsdf_roughdielectric with HostBsdf's sample / eval."""

    def __init__(self, oracle, bp, st):
        self.o, self.bp, self.st = oracle, bp, st

    def sample(self, wi, u):
        return self.o.bsdf_roughdielectric(self.bp, self.st, wi, u=u)

    def eval(self, wi, wo):
        return self.o.bsdf_roughdielectric(self.bp, self.st, wi, wo=wo)[1:]


def test_oracle_roughdielectric_equals_host_bitwise(pkg, oracle, scenes):
    """Sample mode (wo, weight, pdf, eta) and eval mode (f, pdf, eta) on the
    rows of test_gpu_roughdielectric.py::test_batch_kernel_equals_host_bitwise
    -- wi.z of 0 and +-1e-4, inside hits beyond the critical angle, u0 of 0 and
    of the largest float below 1, u2 == F and the next float above it -- and
    eval at the sampled direction, at independent ones on either side and at
    wo.z == 0."""
    rng, bp, st, host, W, U = edge_rows(pkg, scenes)
    orc = OracleBsdf(oracle, bp, st)
    mism = n_void = n_enter = n_leave = 0
    WO = np.zeros_like(W)
    for i, (w, u) in enumerate(zip(W, U)):
        a, b = host.sample(w, u), orc.sample(w, u)
        mism += not _same(a, b)
        WO[i] = a[0]
        n_void += a[2] == 0.0
        n_enter += np.float32(a[3]) == bp[4]
        n_leave += np.float32(a[3]) == bp[5]
    print(f"oracle roughdielectric sample vs host: {mism} of {len(W)} rows differ; {n_void} void, {n_enter} entering, "
          f"{n_leave} leaving")
    assert mism == 0
    assert n_void > 50 and n_enter > 500 and n_leave > 300
    WO[::3] = sphere_wi(rng, len(WO[::3]), 0.0)
    WO[5] = (0.0, 1.0, 0.0)                                # wo.z == 0
    WO[7] = (0.6, 0.0, 0.8)
    WO[8] = (0.6, 0.0, -0.8)
    mism = n_pos = n_trans = 0
    for w, o in zip(W, WO):
        a, b = host.eval(w, o), orc.eval(w, o)
        mism += not _same(a, b)
        n_pos += a[1] > 0
        n_trans += a[1] > 0 and w[2] * o[2] < 0
    print(f"oracle roughdielectric eval vs host: {mism} rows differ; {n_pos} with pdf > 0, {n_trans} of them "
          f"transmitted")
    assert mism == 0 and n_pos > 2000 and n_trans > 500
    assert orc.eval(W[0], WO[0])[1] == 0.0                 # wi.z == 0


@pytest.mark.parametrize("alpha", [0.05, 0.2, 0.5])
def test_oracle_roughdielectric_matches_float64(pkg, oracle, scenes, alpha):
    """The oracle through test_host_matches_float64's body, unchanged; its
    exempt share is not above the host's on the same rows."""
    share_o = check_matches_float64(lambda bp, st: OracleBsdf(oracle, bp, st), scenes, alpha, who="oracle")
    share_h = check_matches_float64(lambda bp, st: HostBsdf(pkg, bp, st), scenes, alpha)
    assert share_o <= share_h


FURNACE_SPP = 32


@pytest.mark.parametrize("flip", [False, True], ids=["front", "back"])
def test_dielectric_furnace_known_answer(oracle, scenes, plog, flip):
    """The pane furnace of tests/test_gpu_roughdielectric.py (R = T = 1) through
    the oracle's Li alone, BSDF only, against the float64 albedo by
    _known_answer's rule.  32 samples a pixel: the standard error (about 6e-4)
    clears SE_MIN, which the helper asserts."""
    import torch
    desc = _furnace(scenes, 1.0, 1.0, flip)
    r = oracle.li_render(desc, *LEAF, spp=FURNACE_SPP, seed=1301, threads=8)
    on_pane = r["hit_bsdf"][0] == 1
    assert on_pane.all() and (r["inside"][0] == (1 if flip else 0)).all()
    _known_answer(scenes, desc, 1.0, 1.0, -1.0 if flip else 1.0, torch.from_numpy(r["image"]),
                  f"oracle_bsdf_{'back' if flip else 'front'}", plog)
    px = r["image"][0].astype(np.float64)
    assert px.std(ddof=1) / np.sqrt(px.size) >= SE_MIN      # (the albedo quadrature is refined to SE_MIN / 4)
    # the saved vertex carries the normal of the side the path came from
    n = r["rec"][13:16, 0][:, r["nv"] > 0]
    assert (n[2] == 1.0).all() and (n[0] == 0).all()


def _glass(scenes, w, h, **kw):
    return scenes.cornell_box(w, h, dielectric=("TallBox",), dielectric_lift=0.02, dielectric_ior=(ETA, 1.0), **kw)


def test_threads_do_not_change_results_dielectric(oracle, scenes):
    desc = _glass(scenes, 32, 18, dielectric_alpha=0.1)
    a = oracle.li_render(desc, *LEAF, spp=2, rr_depth=3, seed=3, threads=1)
    b = oracle.li_render(desc, *LEAF, spp=2, rr_depth=3, seed=3, threads=5)
    for k in ("image", "image_sqr", "rec", "nv", "hit_bsdf", "inside"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert (a["inside"] == 1).sum() > 10 and (a["nv"] > 3).any()
    # the path's relative index enters roulette: the same render with it forced to 1 differs
    c = oracle.li_render(desc, *LEAF, spp=2, rr_depth=3, seed=3, threads=5, rr_eta_one=True)
    assert not np.array_equal(a["nv"], c["nv"]) or not np.array_equal(a["rec"], c["rec"])
    # and a glass scene is not rendered as a diffuse one
    d2 = dict(desc)
    del d2["bsdf_params"], d2["learned_models_nd"]
    e = oracle.li_render(d2, *LEAF, spp=2, rr_depth=3, seed=3, threads=5)
    assert (e["inside"] <= 0).all() and not np.array_equal(a["rec"], e["rec"])


def test_dielectric_product_conditional_equals_host_bitwise(pkg, oracle, scenes):
    """RoughDielectric::getDMM's conditional (the shipped SDMM5 at (theta_i,
    alpha, eta), pruned to 2, no forced component) through
    or_learned_nd_conditional == sdmm_learned_conditional on every bit."""
    model = scenes.load_learned_nd(scenes.LEARNED_DIELECTRIC)
    L = pkg.LearnedBSDFND(*model)
    rng = np.random.default_rng(41)
    dirs = [w for w in sphere_wi(rng, 60)] + [np.float32([0.0, 0.0, 1.0]), np.float32([1.0, 0.0, 0.0]),
                                             np.float32([0.0, np.sqrt(1 - 1e-8), 1e-4])]
    n2 = 0
    for alpha in (0.05, 0.1, 0.3):
        bp, _ = scenes.dielectric_params(int_ior=ETA, ext_ior=1.0, alpha=alpha)
        rest = (float(bp[6]), float(bp[4]))
        for wl in dirs:
            a = L.conditional(rest, wl, 2, -1)
            b = oracle.learned_nd_conditional(model, rest, wl, 2, -1)
            assert _same(a, b), (alpha, wl)
            assert (len(b[0]) == 0) == (not wl[2] > 0)     # (none from inside: roughdielectric.cpp:199)
            n2 += len(b[0]) == 2
    assert n2 > 60
