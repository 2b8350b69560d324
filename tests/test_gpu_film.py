"""GPU: the device film (film.hip) against the host film, bit for bit (NaNs
matching NaNs): the per-pixel variance, every pass's statistics, the combined
estimate after every included pass, and the errors.  The host film itself is
held to the numpy restatement in tests/test_film.py.

Shapes: pixel counts around the wave (63, 64, 65) and the reduction's chunk of
256 (255, 256, 257), one pixel, rows and columns, an odd image (67 x 131: the
scalar path over many chunks), 300 x 300 (the 16-byte path, 352 chunks per
channel: a second reduction level) and planes that are not 16-byte aligned.
"""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import film_cases as fc  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 63), (64, 1), (1, 65), (255, 1), (1, 256), (257, 1), (67, 131), (300, 300)]
SPPS = (4, 2, 7, 3, 64, 5, 4)
FIRST = 4

_cache = {}


def _inputs(shape):
    """Seven planted passes and a ground truth of one shape, made once."""
    if ("in", shape) not in _cache:
        h, w = shape
        _cache[("in", shape)] = ([fc.make_pass(h, w, 300 + i, planted=True) + (SPPS[i], i) for i in range(7)],
                                 fc.make_truth(h, w, 9))
    return _cache[("in", shape)]


def _host(pkg, shape, mode):
    """The host film over _inputs(shape), run once per (shape, mode)."""
    key = ("host", shape, mode)
    if key not in _cache:
        passes, gt = _inputs(shape)
        h, w = shape
        film = pkg.Film(w, h, mode, FIRST, device=-1)
        r = {"variance": film.variance(*passes[0][:3]), "stats": [], "resolve": {}, "errors": {}, "individual": []}
        for img, sqr, spp, it in passes:
            r["stats"].append(film.add_pass(img, sqr, spp, it))
            r["individual"].append(film.errors(gt, img))
            if it >= FIRST:
                r["resolve"][it] = film.resolve()
                r["errors"][it] = film.errors(gt)
        _cache[key] = r
    return _cache[key]


def _same_stats(a, b):
    return (np.array_equal(fc.bits64(a["pcv"]), fc.bits64(b["pcv"])) and a["included"] == b["included"]
            and np.array_equal(fc.bits64(a["mean_pixel_variance"]), fc.bits64(b["mean_pixel_variance"])))


def _same_errors(a, b):
    return all(np.array_equal(fc.bits64(a[k]), fc.bits64(b[k])) for k in ("MrSE", "MAPE", "SMAPE"))


def _dev(a, gpu, misalign=False):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(gpu)
    if not misalign:
        return t
    buf = torch.empty(t.numel() + 1, device=gpu)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def _check_film(pkg, gpu, shape, mode, misalign=False):
    import torch
    passes, gt = _inputs(shape)
    want = _host(pkg, shape, mode)
    h, w = shape
    film = pkg.Film(w, h, mode, FIRST, device=0)
    gtd = _dev(gt, gpu, misalign)
    img, sqr, spp, _ = passes[0]
    out = _dev(np.zeros_like(img), gpu, misalign)
    got = film.variance(_dev(img, gpu, misalign), _dev(sqr, gpu, misalign), spp, out=out)
    assert np.array_equal(fc.bits(got.cpu().numpy()), fc.bits(want["variance"]))
    for k, (img, sqr, spp, it) in enumerate(passes):
        di, ds = _dev(img, gpu, misalign), _dev(sqr, gpu, misalign)
        st = film.add_pass(di, ds, spp, it)
        assert _same_stats(st, want["stats"][k]), (shape, mode, it, st, want["stats"][k])
        assert _same_errors(film.errors(gtd, di), want["individual"][k]), (shape, mode, it)
        if it >= FIRST:
            res = film.resolve(out=out)
            assert np.array_equal(fc.bits(res.cpu().numpy()), fc.bits(want["resolve"][it])), (shape, mode, it)
            assert _same_errors(film.errors(gtd), want["errors"][it]), (shape, mode, it)
        else:
            with pytest.raises(pkg.SDMMError, match="-3"):
                film.resolve(out=out)
    assert len(film) == 7
    assert all(_same_stats(film.pass_stats(k), want["stats"][k]) for k in range(7))
    torch.cuda.synchronize()


@pytest.mark.parametrize("mode", fc.MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_film_is_the_host_film(pkg, gpu, shape, mode):
    _check_film(pkg, gpu, shape, mode)


@pytest.mark.parametrize("mode", fc.MODES)
def test_unaligned_planes(pkg, gpu, mode):
    """npix a multiple of 4 but planes 4 bytes off a 16-byte boundary: the scalar path."""
    _check_film(pkg, gpu, (1, 256), mode, misalign=True)
    _check_film(pkg, gpu, (300, 300), mode, misalign=True)


def test_grid_stride_loops(pkg, gpu):
    """1700 x 1700: more chunks (33 870) than the reducing kernels have waves
    and more quads than the streaming kernels have threads, so every kernel's
    grid-stride loop runs more than once; three reduction levels."""
    shape = (1700, 1700)
    img, sqr = fc.make_pass(*shape, 77, planted=True)
    gt = fc.make_truth(*shape, 78)
    films = [pkg.Film(shape[1], shape[0], "max_var", 0, device=d) for d in (-1, 0)]
    data = [(img, sqr, gt), tuple(_dev(a, gpu) for a in (img, sqr, gt))]
    got = []
    for f, (i, s, g) in zip(films, data):
        st = [f.add_pass(i, s, 4, 0), f.add_pass(s, i, 3, 1)]
        res = f.resolve()
        got.append((st, f.errors(g), f.errors(g, i), res if f.device < 0 else res.cpu().numpy()))
    (hs, he, hi, hr), (ds, de, di, dr) = got
    assert all(_same_stats(a, b) for a, b in zip(hs, ds))
    assert _same_errors(he, de) and _same_errors(hi, di)
    assert np.array_equal(fc.bits(hr), fc.bits(dr))
    assert np.isfinite(hs[0]["pcv"][2]) and hs[0]["pcv"][2] > 0


def test_planted_pixels_reach_the_device(pkg, gpu):
    """The inputs above do carry the non-finite pattern (the comparison is not NaN against NaN throughout)."""
    want = _host(pkg, (67, 131), "uniform")
    v = want["variance"].reshape(3, -1)
    p = fc.planted_pixels(67 * 131)
    assert np.isnan(v[0, p[0]]) and v[2, p[3]] == 2000.0 and np.isfinite(v[2]).all()
    final = want["resolve"][6]
    assert np.isfinite(final[2]).all() and np.isnan(final[0]).any() and np.isinf(final[1]).any()
    assert np.isfinite(_host(pkg, (67, 131), "var")["resolve"][6][2]).all()


@pytest.mark.parametrize("mode", fc.MODES)
def test_async_passes_equal_synchronising_passes(pkg, gpu, mode):
    """add_pass with pass_stats = NULL for every pass, then one resolve: no
    host synchronisation in between, the same bits."""
    import torch
    shape = (67, 131)
    passes, gt = _inputs(shape)
    want = _host(pkg, shape, mode)
    film = pkg.Film(shape[1], shape[0], mode, FIRST, device=0)
    dev = [(_dev(i, gpu), _dev(s, gpu), spp, it) for i, s, spp, it in passes]
    for di, ds, spp, it in dev:
        assert film.add_pass(di, ds, spp, it, sync=False) is None
    res = film.resolve()
    torch.cuda.synchronize()
    assert np.array_equal(fc.bits(res.cpu().numpy()), fc.bits(want["resolve"][6]))
    assert all(_same_stats(film.pass_stats(k), want["stats"][k]) for k in range(7))
    assert _same_errors(film.errors(_dev(gt, gpu)), want["errors"][6])
    film.reset()
    assert len(film) == 0
    film.add_pass(dev[5][0], dev[5][1], dev[5][2], 5, sync=False)
    one = pkg.Film(shape[1], shape[0], mode, FIRST, device=-1)
    one.add_pass(passes[5][0], passes[5][1], passes[5][2], 5)
    assert np.array_equal(fc.bits(film.resolve().cpu().numpy()), fc.bits(one.resolve()))


def test_two_films_on_two_streams(pkg, gpu):
    import torch
    shapes = ((67, 131), (300, 300))
    modes = ("max_var", "var")
    streams = [torch.cuda.Stream(gpu) for _ in shapes]
    films = [pkg.Film(s[1], s[0], m, FIRST, device=0) for s, m in zip(shapes, modes)]
    dev = [[(_dev(i, gpu), _dev(q, gpu), spp, it) for i, q, spp, it in _inputs(s)[0]] for s in shapes]
    outs = [f._out() for f in films]
    torch.cuda.synchronize()
    for k in range(7):
        for f, st, d in zip(films, streams, dev):
            f.add_pass(d[k][0], d[k][1], d[k][2], d[k][3], stream=st.cuda_stream, sync=False)
    for f, st, o in zip(films, streams, outs):
        f.resolve(out=o, stream=st.cuda_stream)
    for st in streams:
        st.synchronize()
    for f, s, m, o in zip(films, shapes, modes, outs):
        want = _host(pkg, s, m)
        assert np.array_equal(fc.bits(o.cpu().numpy()), fc.bits(want["resolve"][6])), (s, m)
        assert all(_same_stats(f.pass_stats(k), want["stats"][k]) for k in range(7)), (s, m)


def test_guided_passes_into_a_film(pkg, scenes, gpu):
    """Six sdmm_guiding_iteration passes of the Cornell box, 32 x 32, spp 4:
    the device planes straight into device films (one per mode), their host
    copies into host films; the estimates agree bit for bit.

    At 4096 paths a pass of this light-starved scene lights a handful of pixels
    and can leave a channel black: its variance is then 0, its weight infinite
    and the `var` / `max_var` estimate NaN, as in the reference.  So the
    `uniform` estimate is the one that must be finite, with a finite, positive
    SMAPE against an spp-256 unguided render; the `var` estimate must be finite
    exactly when no included pass had a zero per-channel variance."""
    import torch
    w = h = 32
    first = 2
    sc = pkg.Scene(scenes.cornell_box(w, h))
    _, _, tmin, tmax = sc.normalization()
    g = pkg.Guiding(tmin, tmax)
    dfilm = {m: pkg.Film(w, h, m, first_iteration=first, device=0) for m in fc.MODES}
    hfilm = {m: pkg.Film(w, h, m, first_iteration=first, device=-1) for m in fc.MODES}
    zero_weight = False
    for it in range(6):
        img = torch.zeros(3, h, w, device=gpu)
        sqr = torch.zeros(3, h, w, device=gpu)
        g.iteration(sc, 4, seed=1 + it, push_seed=1001 + it, image=img, image_sqr=sqr)
        torch.cuda.synchronize()
        hi, hq = img.cpu().numpy(), sqr.cpu().numpy()
        for m in fc.MODES:
            ds = dfilm[m].add_pass(img, sqr, 4, it)
            hs = hfilm[m].add_pass(hi, hq, 4, it)
            assert _same_stats(ds, hs) and ds["included"] == (it >= first)
            assert np.isfinite(ds["mean_pixel_variance"])
        zero_weight |= it >= first and bool((ds["pcv"].astype(np.float32) == 0).any())
        print("pass", it, "lit values", int((hi != 0).sum()), "pcv", ds["pcv"])
    tree = pkg.STree(tmin, tmax)
    tree.split_to_depth(2)
    truth, _, _ = sc.render(tree, None, spp=256, guided=False, seed=4242)
    torch.cuda.synchronize()
    est = {}
    for m in fc.MODES:
        est[m] = dfilm[m].resolve().cpu().numpy()
        assert np.array_equal(fc.bits(est[m]), fc.bits(hfilm[m].resolve())), m
        assert _same_errors(dfilm[m].errors(truth), hfilm[m].errors(truth.cpu().numpy())), m
    assert np.isfinite(est["uniform"]).all() and est["uniform"].max() > 0
    assert bool(np.isfinite(est["var"]).all()) == (not zero_weight)
    e = dfilm["uniform"].errors(truth)
    assert np.isfinite(e["SMAPE"]) and e["SMAPE"] > 0
    print("SMAPE of the uniform estimate of passes 2..5 against 256 spp:", e["SMAPE"], "zero weight:", zero_weight)
