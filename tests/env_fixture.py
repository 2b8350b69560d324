"""The environment tests' shared fixture (tests/test_env.py, tests/
test_gpu_env.py): lat-long maps of random texels in [0.1, 2) -- 8x4, 16x8, 1x1,
1x4 (the horizontal wrap with w = 1) and 4x1 (the vertical clamp with h = 1),
width x height -- and the directions: 4096 random unit vectors plus the
hand-placed ones, and numpy restatements of the lookup (envmap.cpp:380-393,
:409; mipmap.h:575-596) at a chosen precision."""
import functools

import numpy as np

SIZES = [(8, 4), (16, 8), (1, 1), (1, 4), (4, 1)]        # (width, height)
N_RANDOM = 4096

# signed permutation matrices: the rotations by 90 degrees about each axis, by
# 180 degrees about x (diag(1, -1, -1)), and a cyclic permutation
ROTATIONS = {
    "rx90": [[1, 0, 0], [0, 0, -1], [0, 1, 0]],
    "ry90": [[0, 0, 1], [0, 1, 0], [-1, 0, 0]],
    "rz90": [[0, -1, 0], [1, 0, 0], [0, 0, 1]],
    "rx180": [[1, 0, 0], [0, -1, 0], [0, 0, -1]],
    "cyc": [[0, 1, 0], [0, 0, 1], [1, 0, 0]],
}


@functools.lru_cache(maxsize=None)
def maps():
    """[(name, pixels [h, w, 3] float32, scale)]"""
    rng = np.random.default_rng(20241020)
    out = []
    for i, (w, h) in enumerate(SIZES):
        out.append((f"{w}x{h}", rng.uniform(0.1, 2.0, (h, w, 3)).astype(np.float32), [1.0, 0.75, 2.5, 1.0, 1.25][i]))
    return out


def desc_of(pixels, scale=1.0, M=None):
    d = {"env_kind": 2, "env_pixels": pixels, "env_scale": scale}
    if M is not None:
        d["env_world_to_local"] = np.asarray(M, np.float32).reshape(-1)
    return d


@functools.lru_cache(maxsize=None)
def directions():
    """(d [n, 3] float32, finite [n] bool): the random unit vectors, then the
    hand-placed directions; the last two are the NaN and the Inf direction."""
    rng = np.random.default_rng(20241021)
    r = rng.normal(size=(N_RANDOM, 3))
    r /= np.linalg.norm(r, axis=-1, keepdims=True)
    f32 = np.float32
    below_one = np.nextafter(f32(1), f32(0))
    side = f32(np.sqrt(1.0 - float(below_one) ** 2))
    tiny = np.asarray([1e-7, 0.0, 1.0]) / np.linalg.norm([1e-7, 0.0, 1.0])
    hand = [
        [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1],       # the axes; +-y are the poles
        [0, 0.6, 0.8], [0, -0.6, 0.8], [-0.0, 0.6, 0.8],                           # the seam: v = (0, ., +1), u = +-0.5
        [0, 0.6, -0.8], [0, -0.6, -0.8],                                           # v = (0, ., -1): u = 0
        tiny, tiny * [-1, 1, 1],                                                   # (+-1e-7, 0, 1) normalised
        [side, below_one, 0], [0, -below_one, side],                               # |v.y| one ulp below 1
        [1.2, 1.6, 0], [0.0, -2.0, 0.0],                                           # length 2: no renormalisation, acos clamps
        [np.nan, np.nan, np.nan], [np.inf, 0.5, -np.inf],
    ]
    d = np.concatenate([r, np.asarray(hand, np.float64)]).astype(np.float32)
    return d, np.isfinite(d).all(-1)


def restate(pixels, scale, M, d, dtype):
    """The lat-long lookup in numpy at `dtype` (float32: every operation
    rounded to float32 with the float32 constants of the reference; float64:
    the formula itself) for finite directions d -> [n, 3] of dtype."""
    T = dtype
    px = np.asarray(pixels, np.float32).astype(T)
    h, w = px.shape[:2]
    M = np.eye(3, dtype=T) if M is None else np.asarray(M, np.float32).reshape(3, 3).astype(T)
    d = np.asarray(d).astype(T)                      # (float64 directions stay float64 at T = float64)
    v = [M[r, 0] * d[:, 0] + M[r, 1] * d[:, 1] + M[r, 2] * d[:, 2] for r in range(3)]
    if T is np.float32:
        inv_2pi, inv_pi = T(0.15915494309189533577), T(0.31830988618379067154)
    else:
        inv_2pi, inv_pi = T(0.5 / np.pi), T(1.0 / np.pi)
    uvx = np.arctan2(v[0], -v[2]).astype(T) * inv_2pi
    uvy = np.arccos(np.minimum(T(1), np.maximum(T(-1), v[1]))).astype(T) * inv_pi
    u, t = uvx * T(w) - T(0.5), uvy * T(h) - T(0.5)
    fx, fy = np.floor(u), np.floor(t)
    x, y = fx.astype(np.int64), fy.astype(np.int64)
    dx1, dy1 = u - fx, t - fy
    dx2, dy2 = T(1) - dx1, T(1) - dy1
    x0, x1 = np.mod(x, w), np.mod(x + 1, w)
    y0, y1 = np.clip(y, 0, h - 1), np.clip(y + 1, 0, h - 1)
    val = (px[y0, x0] * dx2[:, None] * dy2[:, None] + px[y1, x0] * dx2[:, None] * dy1[:, None]
           + px[y0, x1] * dx1[:, None] * dy2[:, None] + px[y1, x1] * dx1[:, None] * dy1[:, None])
    out = val * T(scale)
    assert out.dtype == T
    return out


def rotate_exact(M, d):
    """M d for a signed permutation matrix, formed as the library forms it
    (three products and two sums in float32, all exact here)."""
    M = np.asarray(M, np.float32)
    d = np.asarray(d, np.float32)
    with np.errstate(invalid="ignore"):
        return np.stack([M[r, 0] * d[:, 0] + M[r, 1] * d[:, 1] + M[r, 2] * d[:, 2] for r in range(3)], -1)
