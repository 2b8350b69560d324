"""Inputs of the film tests and a numpy float32 restatement of what the film
computes (include/sdmm_gpu.h, sdmm_film_*; csrc/film.h): the per-pixel variance
of a pass, the three weighting heuristics, the running combination and the
error terms, written the way the reference's scripts write them, in the
float32 arithmetic numpy runs them in.  The means are NOT restated bit for bit:
the library sums in fp64 in a fixed order, the tests hold them to the bound of
sum_bound() against numpy's fp64 mean of the same float32 terms.
"""
import numpy as np

CHUNK = 256          # csrc/film.h: kFilmChunk
MODES = ("var", "max_var", "uniform")


def planted_pixels(npix):
    """Four pixel indices: in the first chunk, on both sides of the first chunk
    boundary, and in the last chunk (folded into the image where it is smaller)."""
    return [i % npix for i in (1, CHUNK - 1, CHUNK, npix - 1)]


def make_pass(h, w, seed, planted=True):
    """(img, sqr) float32 (3, h, w): values log-uniform over 1e-3 .. 50, the
    squares image 1 .. 4 times img^2.  planted: a NaN (channel 0) and a +inf
    (channel 1) in img, a sqr of 0 and a sqr of 1e9 (the clip to 2000 is
    reached) in channel 2, at planted_pixels()."""
    rng = np.random.default_rng(seed)
    img = np.exp(rng.uniform(np.log(1e-3), np.log(50.0), (3, h * w))).astype(np.float32)
    sqr = (img * img * rng.uniform(1.0, 4.0, (3, h * w)).astype(np.float32)).astype(np.float32)
    if planted:
        p = planted_pixels(h * w)
        img[0, p[0]] = np.nan
        img[1, p[1]] = np.inf
        sqr[2, p[2]] = 0.0
        sqr[2, p[3]] = 1e9
    return img.reshape(3, h, w), sqr.reshape(3, h, w)


def make_truth(h, w, seed):
    rng = np.random.default_rng(seed)
    return np.exp(rng.uniform(np.log(1e-3), np.log(50.0), (3, h, w))).astype(np.float32)


def bits(a):
    """Bit patterns, every NaN folded onto one (host and device NaN payloads differ)."""
    a = np.ascontiguousarray(a, np.float32)
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = 0x7FC00000
    return b


def bits64(a):
    a = np.ascontiguousarray(a, np.float64)
    b = a.view(np.uint64).copy()
    b[np.isnan(a)] = 0x7FF8000000000000
    return b


def to_hwc(a):
    """(3, H, W) planes -> the (H, W, 3) layout the reference's scripts hold."""
    return np.ascontiguousarray(np.moveaxis(np.asarray(a, np.float32), 0, -1))


def to_planes(a):
    return np.ascontiguousarray(np.moveaxis(a, -1, 0))


def np_variance(img, sqr, spp):
    """The clipped per-pixel variance, on (H, W, 3) float32 arrays; spp a Python int."""
    with np.errstate(all="ignore"):
        v = spp / (spp - 1) * (sqr / spp - (img / spp) ** 2)
        v = np.clip(v, 0, 2000)
    assert v.dtype == np.float32
    return v


class NumpyFilm:
    """The combination loop on (H, W, 3) float32 arrays, given each pass's
    per-channel variance (so that the fp64-mean departure stays out of it)."""

    def __init__(self, mode, first_iteration=4):
        self.mode, self.first = mode, first_iteration
        self.final, self.recip = None, 0.0

    def add_pass(self, img, sqr, spp, iteration, pcv32):
        if iteration < self.first:
            return False
        with np.errstate(all="ignore"):
            if self.mode == "var":
                weight = np.asarray(pcv32, np.float32)
            elif self.mode == "max_var":
                weight = np.maximum(np_variance(img, sqr, spp), np.asarray(pcv32, np.float32))
            else:
                weight = 1 / spp
            self.recip = self.recip + 1.0 / weight
            if self.final is None:
                self.final = img / weight
            else:
                self.final = self.final + img / weight
        assert self.final.dtype == np.float32
        return True

    def resolve(self):
        with np.errstate(all="ignore"):
            out = self.final / self.recip
        assert out.dtype == np.float32
        return out


def np_error_terms(a, g):
    """The elementwise float32 terms of MrSE, MAPE, SMAPE (before any mean)."""
    with np.errstate(all="ignore"):
        ac, gc = np.clip(a, 0, 1), np.clip(g, 0, 1)
        t0 = (ac - gc) ** 2 / (1e-2 + gc ** 2)
        t1 = abs(a - g) / (1e-2 + g)
        t2 = 2 * abs(a - g) / (1e-2 + g + a)
    assert t0.dtype == t1.dtype == t2.dtype == np.float32
    return t0, t1, t2


def sum_bound(n):
    """Relative distance between two orderings of an fp64 sum of n non-negative
    terms: each is within (n - 1) 2^-53 of the exact sum."""
    return 2.0 * (n - 1) * 2.0 ** -53


def close(got, ref, n):
    """got within sum_bound(n) of ref (relative), NaN matching NaN, inf matching inf."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    if not np.array_equal(bits64(got[~fin]), bits64(ref[~fin])):
        return False
    return bool(np.all(np.abs(got[fin] - ref[fin]) <= sum_bound(n) * np.abs(ref[fin])))
