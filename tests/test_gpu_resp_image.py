"""The split responsibility kernel's cached coefficient image.

estep_resp_split_kernel copies one prebuilt coefficient image per mixture into
LDS; estep_resp_image_kernel builds that image on the first
sdmm_responsibilities after a change of the parameters.  With
SDMM_RESP_IMAGE=inline (read when a handle is created) every workgroup builds
the image itself, as before the image was cached.  Checked here, on mixture
pairs with the same parameters, one created under each setting:

  * the cached path's posterior equals the inline one's byte for byte, at the
    edges of the deal and in every configuration (R = 1, 2, 4, 8 and K < Kp);
  * every entry point that writes a handle's parameters invalidates its image:
    after each step of one deterministic sequence the two outputs are byte
    identical, and the handle's builder launches count the parameter changes
    and not the calls;
  * the image belongs to the handle: two mixtures alternating on one stream
    each equal their own inline twin.

Every batch carries hpdf and the isDiffuse bytes (half of them set).
"""
import contextlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WPB = 12          # waves per workgroup of the K = 128 configuration


@contextlib.contextmanager
def _env(inline, K):
    """The environment a handle of this test is created under (the library
    reads both switches at creation): the split kernel for every K, and the
    image setting."""
    keep = {k: os.environ.get(k) for k in ("SDMM_RESP_IMAGE", "SDMM_RESP_KERNEL")}
    try:
        if inline:
            os.environ["SDMM_RESP_IMAGE"] = "inline"
        else:
            os.environ.pop("SDMM_RESP_IMAGE", None)
        if K <= 64:
            os.environ["SDMM_RESP_KERNEL"] = "split"
        yield
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _host_params(pkg, synth, b, K, seed):
    """K components of a host hemisphere initialisation (8 per seed point: the
    first K of the next multiple's, weights renormalised)."""
    Kg = 8 * ((K + 7) // 8)
    pos, nrm = synth.model_seed_points(b, Kg)
    h = pkg.hemisphere_init_host(pos, nrm, synth.DEPTH_PRIOR, synth.SPATIAL_DISTANCE, seed)
    return h["weights"][:K] / h["weights"][:K].sum(), h["mean"][:K], h["cov"][:K]


def _pair(pkg, synth, b, K, seed=None):
    """(cached, inline): two handles with the same parameters."""
    seed = synth.SEED_MODEL if seed is None else seed
    out = []
    for inline in (False, True):
        with _env(inline, K):
            mix = pkg.SDMM(K)
        if K % 8 == 0:
            pos, nrm = synth.model_seed_points(b, K)
            mix.init_hemisphere(pos, nrm, synth.DEPTH_PRIOR, synth.SPATIAL_DISTANCE, seed)
        else:
            mix.set_params(*_host_params(pkg, synth, b, K, seed))
        name = mix.kernel_name("resp")
        assert "split" in name and ("inline" in name) == inline, name
        out.append(mix)
    return out


def _samples(pkg, b, a=0, e=None):
    e = b["w"].shape[0] if e is None else e
    return pkg.DeviceSamples.from_numpy(b["x"][:, a:e], b["w"][a:e], b["hpdf"][a:e], b["is_diffuse"][a:e])


def _bits(mix, ds, K, gpu):
    import torch
    resp = torch.full((ds.n, K), -1.0, device=gpu)
    mix.posterior(ds, resp)
    torch.cuda.synchronize()
    return resp.cpu().numpy().view(np.uint32)


def _same(cached, inline, ds, K, gpu, what=""):
    got, ref = _bits(cached, ds, K, gpu), _bits(inline, ds, K, gpu)
    diff = np.flatnonzero((got != ref).any(1))
    assert diff.size == 0, f"{what}: {diff.size} of {ds.n} rows differ from the inline build, first {diff[:8]}"
    assert (ref != np.float32(-1.0).view(np.uint32)).all(), f"{what}: rows never written"
    return ref


def _builds(mix):
    return mix.layout()["resp_image_builds"]


def _big_n(gpu):
    import torch
    W = WPB * torch.cuda.get_device_properties(gpu).multi_processor_count
    return 16 * (2 * W + W // 3 + 5) + 7


_k128 = {}


def _k128_case(pkg, synth, gpu):
    if not _k128:
        n = _big_n(gpu)
        b = synth.em_batch(n, 128, heuristic=True)
        _k128["b"] = b
        _k128["pair"] = _pair(pkg, synth, b, 128)
    return _k128["b"], _k128["pair"]


@pytest.mark.parametrize("n", [1, 17, 16 * WPB + 1, "two_rounds"])
def test_cached_equals_inline_k128(pkg, synth, gpu, n):
    """K = 128 (R = 8, rows staged through LDS): one partial tile, two tiles,
    one workgroup and a tile, and just above two rounds of resident waves."""
    b, (cached, inline) = _k128_case(pkg, synth, gpu)
    n = _big_n(gpu) if n == "two_rounds" else n
    ref = _same(cached, inline, _samples(pkg, b, 0, n), 128, gpu, f"n={n}")
    assert np.isfinite(ref.view(np.float32)).all() and ref.view(np.float32).sum() > 0
    assert _builds(inline) == 0 and _builds(cached) == 1   # one image for every launch of this module's pair


@pytest.mark.parametrize("K", [16, 32, 64, 100])
def test_cached_equals_inline_other_configurations(pkg, synth, gpu, K):
    """R = 1, 2, 4 (the image is 8, 16, 32 KB) and K = 100 below Kp = 128 (dead
    padded components in the image)."""
    n = 1000
    b = synth.em_batch(n, 128, heuristic=True)
    cached, inline = _pair(pkg, synth, b, K)
    ref = _same(cached, inline, _samples(pkg, b), K, gpu, f"K={K}")
    assert ref.view(np.float32).sum() > 0
    assert _builds(cached) == 1 and _builds(inline) == 0


def test_every_parameter_writer_invalidates_the_image(pkg, synth, gpu, tmp_path):
    """One operation sequence on a cached and an inline mixture (and a second
    pair for the batched entry points): byte-identical posteriors after every
    step, one builder launch per parameter change."""
    import torch
    K, n = 128, 1000
    b = synth.em_batch(n, 128, heuristic=True)
    ds = _samples(pkg, b)
    seg = np.array([0, n // 2, n], np.int64)
    pos, nrm = synth.model_seed_points(b, K)
    A = _pair(pkg, synth, b, K)            # (cached, inline)
    B = _pair(pkg, synth, b, K, seed=77)   # the second mixture of the batched steps
    want = {"A": 0, "B": 0}

    def check(what, **changed):
        """posterior of both pairs; the listed pairs' images were invalidated once"""
        for name, pair in (("A", A), ("B", B)):
            _same(pair[0], pair[1], ds, K, gpu, what)
            want[name] += changed.get(name, 0)
            assert _builds(pair[0]) == want[name], f"{what}: {name} built {_builds(pair[0])} images, {want[name]} changes"
            assert _builds(pair[1]) == 0

    check("first use", A=1, B=1)
    for m in A:
        m.init_hemisphere(pos, nrm, synth.DEPTH_PRIOR, synth.SPATIAL_DISTANCE, 99)
    check("init_hemisphere", A=1)
    prm = _host_params(pkg, synth, b, K, 5)
    for m in A:
        m.set_params(*prm)
    check("set_params", A=1)
    saved = [(m.get_params(), m.get_state()) for m in A]
    for m in A:
        m.optimize(ds)
    check("optimize", A=1)
    for m in A:
        stats = torch.zeros(pkg.stats_len(K), dtype=torch.float64, device=gpu)
        m.estep_stats(ds, stats)
        m.mstep(stats, n)
    check("estep_stats + mstep", A=1)
    for m, (p, _) in zip(A, saved):
        m.restore_params(p)
    check("restore_params", A=1)
    for m, (_, st) in zip(A, saved):
        m.set_state(st)
    check("set_state", A=1)
    for i in range(2):
        pkg.em_step_batched([A[i], B[i]], ds, seg, 2)
    check("em_step_batched", A=1, B=1)
    for i in range(2):
        pkg.init_hemisphere_batched([A[i], B[i]], np.stack([pos, pos[::-1]]), np.stack([nrm, nrm[::-1]]),
                                    synth.DEPTH_PRIOR, synth.SPATIAL_DISTANCE, [3, 4])
    check("init_hemisphere_batched", A=1, B=1)

    # new handles: a clone and a loaded checkpoint build their own image, the
    # source keeps its own
    clones, loaded = [], []
    for i, inline in enumerate((False, True)):
        with _env(inline, K):
            clones.append(A[i].clone())
            A[i].save_json(tmp_path / f"m{i}.json")
            loaded.append(pkg.SDMM.load_json(tmp_path / f"m{i}.json"))
    for what, pair in (("clone", clones), ("load_json", loaded)):
        ref = _same(pair[0], pair[1], ds, K, gpu, what)
        assert np.array_equal(ref, _bits(A[1], ds, K, gpu)), f"{what}: not the source's posterior"
        assert _builds(pair[0]) == 1 and _builds(pair[1]) == 0
    check("clone + load_json leave the source alone")

    comm = pkg.Comm.host(1, 0, lambda a: None, lambda a, root: None)
    for m in A:
        m.optimize_sharded(comm, ds)
    check("optimize_sharded", A=1)
    for i in range(2):
        pkg.mix_broadcast([A[i], B[i]], [0, 0], comm)
    check("mix_broadcast", A=1, B=1)
    comm.close()

    for _ in range(10):
        check("repeated posterior")


def test_two_mixtures_alternate_on_one_stream(pkg, synth, gpu):
    """The image is per handle: two cached mixtures with different parameters
    served in turn on one stream each equal their own inline twin."""
    K, n = 128, 16 * WPB * 3 + 5
    b = synth.em_batch(n, 128, heuristic=True)
    ds = _samples(pkg, b)
    P, Q = _pair(pkg, synth, b, K), _pair(pkg, synth, b, K, seed=12345)
    refs = [_bits(P[1], ds, K, gpu), _bits(Q[1], ds, K, gpu)]
    assert not np.array_equal(refs[0], refs[1])
    for turn in range(3):
        for pair, ref in ((P, refs[0]), (Q, refs[1])):
            assert np.array_equal(_bits(pair[0], ds, K, gpu), ref), f"turn {turn}"
    assert _builds(P[0]) == 1 and _builds(Q[0]) == 1
