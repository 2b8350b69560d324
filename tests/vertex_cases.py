"""Constructed path vertices for the training-data producer and the guiding
model's pools (sdmm_push_training, sdmm_guiding_push): a sdmm_path_vertices is
a plain struct of device pointers, so no scene is needed.

Builders (numpy only; the GPU enters through device_vertices / device_tree):

  make_vertices    the record planes rec[(f*V + v)*P + p] (fields 0-2 weight,
                   3-5 throughput, 6 pdf, 7-12 point, 13-15 normal) and nv
  device_vertices  a pkg.PathVertices over two torch tensors it keeps alive
  unit_tree        the unit cube split to a depth, as the oracle builds it
  device_tree      a pkg.STree holding exactly those node arrays

Families (seeded, over the unit-cube tree; family(oracle, name) builds one of
FAMILIES with its tree):

  mixed        every weight class (3000 everywhere, a NaN channel, an inf
               channel, (+inf, -inf, 1), three finite channels whose sum
               overflows, an average of exactly 1000.0f and of the next average
               the expression can give) and every position class (outside,
               NaN, on the tree's max faces, on the 1/64 lattice of the split
               planes), nv anywhere in 0..V
  single_leaf  mixed on the depth-0 tree: every jitter draw finds the same
               leaf, all 8 attempts fail, no jitter record
  corner       nv = 1 at (1e-4, 1e-4, 1e-4) of the depth-1 tree: every draw
               lands in the same leaf or outside the tree
  eighth_draw  nv = 1 where one draw in eight leaves the leaf: paths whose first
               success is the eighth draw, the last the 8-attempt rule allows
  deep         a tree split by clustered positions with a small threshold
               (leaf sizes over several decades), vertices from the same clusters

nv[p] stays within 0..V: the library trusts it (make_vertices asserts it).
"""
import numpy as np

N_FIELDS = 16
LO = np.zeros(3, np.float32)
HI = np.ones(3, np.float32)

# weight classes of `mixed`
W_PLAIN, W_3000, W_NAN, W_INF, W_INF_MINUS_INF, W_OVERFLOW, W_1000, W_1000_NEXT = range(8)
WEIGHT_CLASSES = {"plain": W_PLAIN, "3000": W_3000, "nan": W_NAN, "inf": W_INF, "inf_minus_inf": W_INF_MINUS_INF,
                  "overflow": W_OVERFLOW, "avg_1000": W_1000, "avg_1000_next": W_1000_NEXT}
# position classes of `mixed`
P_PLAIN, P_OUTSIDE, P_NAN, P_MAXFACE, P_LATTICE = range(5)
POSITION_CLASSES = {"plain": P_PLAIN, "outside": P_OUTSIDE, "nan": P_NAN, "max_face": P_MAXFACE,
                    "lattice": P_LATTICE}


def average(w):
    """Spectrum::average as the producer forms it, in float32: (a + b + c) * (1/3)."""
    w = np.asarray(w, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        return ((w[..., 0] + w[..., 1]) + w[..., 2]) * (np.float32(1.0) / np.float32(3.0))


def boundary_triples():
    """(t1000, tnext): float32 weight triples whose average is exactly 1000.0f
    (no second jitter: the rule is a strict >) and the smallest average above
    it that the expression can give -- the triple's sum is the float after the
    first triple's sum.  (Sums near 3000 are 2^-12 apart, a third of which is
    more than the 2^-14 between floats near 1000, so nextafter(1000) itself is
    not a value of the expression there; asserted below.)"""
    t0 = np.array([1000.0, 1000.0, 1000.0], np.float32)
    t1 = np.array([1000.0, 1000.0, np.float32(1000.0) + np.float32(2.0 ** -12)], np.float32)
    s0 = (t0[0] + t0[1]) + t0[2]
    s1 = (t1[0] + t1[1]) + t1[2]
    assert s0 == np.float32(3000.0) and s1 == np.nextafter(s0, np.float32(np.inf))
    a0, a1 = average(t0), average(t1)
    assert a0 == np.float32(1000.0), a0
    assert a1 > np.float32(1000.0) and a1 <= np.nextafter(np.nextafter(a0, np.float32(np.inf)), np.float32(np.inf)), a1
    return t0, t1


def make_vertices(P, V, nv, pos, weight, wo=None, normal=None):
    """pos, weight, wo, normal: (P, V, 3).  Returns (rec, nv) in the library's
    layout; throughput and pdf are 1 (the producer does not read them)."""
    nv = np.ascontiguousarray(nv, np.int32).reshape(P)
    assert ((nv >= 0) & (nv <= V)).all(), "nv must stay within 0..V: the library trusts it"
    r = np.zeros((N_FIELDS, V, P), np.float32)
    r[3:7] = 1.0

    def put(f0, a):
        a = np.asarray(a, np.float32).reshape(P, V, 3)
        r[f0:f0 + 3] = a.transpose(2, 1, 0)

    put(0, weight)
    put(7, pos)
    if wo is None:
        wo = np.zeros((P, V, 3), np.float32)
        wo[..., 2] = 1.0
    put(10, wo)
    if normal is None:
        normal = np.zeros((P, V, 3), np.float32)
        normal[..., 2] = 1.0
    put(13, normal)
    return np.ascontiguousarray(r.reshape(-1)), nv


def device_vertices(pkg, rec, nv, V, path0, gpu):
    """A pkg.PathVertices whose struct points at two torch tensors (kept alive
    by the object, in the slot a render's scene takes)."""
    import torch
    P = int(nv.shape[0])
    assert rec.shape == (N_FIELDS * V * P,) and ((nv >= 0) & (nv <= V)).all()
    trec = torch.from_numpy(np.ascontiguousarray(rec, np.float32)).to(gpu)
    tnv = torch.from_numpy(np.ascontiguousarray(nv, np.int32)).to(gpu)
    torch.cuda.synchronize()
    s = pkg._PathVertices()
    s.n_paths, s.max_vertices, s.path0 = P, int(V), int(path0)
    s.rec = trec.data_ptr() if P else None
    s.nv = tnv.data_ptr() if P else None
    return pkg.PathVertices(s, (trec, tnv), gpu.index or 0)


def unit_tree(oracle, depth):
    """(aabb, child, axis) of the unit cube split to `depth` (8^depth leaves)."""
    e = np.zeros(0, np.float32)
    return oracle.stree_build(LO, HI, depth, [e, e, e], 0)


def device_tree(pkg, nodes):
    t = pkg.STree(LO, HI)
    t.set_nodes(*nodes)
    return t


def visited(nv, V, saved):
    """(P, V) mask of the vertices the producer visits: nv - saved <= v < nv."""
    v = np.arange(V)[None, :]
    return (v < nv[:, None]) & (v >= nv[:, None] - saved)


def _directions(rng, shape):
    d = rng.normal(size=shape + (3,))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return d.astype(np.float32)


def mixed(P=1000, seed=11, V=9, boundary="both"):
    """boundary: which of the two near-1000 triples the W_1000 / W_1000_NEXT
    vertices carry -- "both" (each its own), "exact" (all the exact one) or
    "next" (all the next one); the three builds differ in those weights only."""
    rng = np.random.default_rng(seed)
    nv = rng.integers(0, V + 1, size=P).astype(np.int32)
    pos = rng.uniform(0.0, 1.0, size=(P, V, 3)).astype(np.float32)
    w = rng.exponential(1.0, size=(P, V, 3)).astype(np.float32)
    t0, t1 = boundary_triples()
    u = rng.uniform(size=(P, V))
    ch = rng.integers(0, 3, size=(P, V))
    wc = np.full((P, V), W_PLAIN, np.int32)
    edges = [(W_3000, 0.10), (W_NAN, 0.05), (W_INF, 0.05), (W_INF_MINUS_INF, 0.01), (W_OVERFLOW, 0.01),
             (W_1000, 0.03), (W_1000_NEXT, 0.03)]
    lo = 0.0
    for c, share in edges:
        wc[(u >= lo) & (u < lo + share)] = c
        lo += share
    w[wc == W_3000] = 3000.0
    one = np.zeros((P, V, 3), bool)
    np.put_along_axis(one, ch[..., None], True, axis=2)
    w[(wc == W_NAN)[..., None] & one] = np.nan
    w[(wc == W_INF)[..., None] & one] = np.inf
    w[wc == W_INF_MINUS_INF] = np.array([np.inf, -np.inf, 1.0], np.float32)
    w[wc == W_OVERFLOW] = np.float32(3e38)
    w[wc == W_1000] = t1 if boundary == "next" else t0
    w[wc == W_1000_NEXT] = t0 if boundary == "exact" else t1
    u = rng.uniform(size=(P, V))
    ch = rng.integers(0, 3, size=(P, V))
    pc = np.full((P, V), P_PLAIN, np.int32)
    lo = 0.0
    for c, share in [(P_OUTSIDE, 0.05), (P_NAN, 0.01), (P_MAXFACE, 0.02), (P_LATTICE, 0.15)]:
        pc[(u >= lo) & (u < lo + share)] = c
        lo += share
    pos[pc == P_OUTSIDE, 0] = 1.5
    one = np.zeros((P, V, 3), bool)
    np.put_along_axis(one, ch[..., None], True, axis=2)
    pos[(pc == P_NAN)[..., None] & one] = np.nan
    pos[(pc == P_MAXFACE)[..., None] & one] = 1.0
    lat = (np.round(pos * 64.0) / 64.0).astype(np.float32)
    pos[pc == P_LATTICE] = lat[pc == P_LATTICE]
    rec, nv = make_vertices(P, V, nv, pos, w, _directions(rng, (P, V)), _directions(rng, (P, V)))
    return {"P": P, "V": V, "rec": rec, "nv": nv, "weight_class": wc, "position_class": pc, "weight": w,
            "pos": pos}


def single_leaf(P=1000, seed=11):
    return mixed(P, seed)


def corner(P=4096, V=2):
    nv = np.ones(P, np.int32)
    pos = np.full((P, V, 3), 1e-4, np.float32)
    w = np.ones((P, V, 3), np.float32)
    rec, nv = make_vertices(P, V, nv, pos, w)
    return {"P": P, "V": V, "rec": rec, "nv": nv, "weight": w, "pos": pos}


EIGHTH_POS = (0.3125, 0.25, 0.25)


def eighth_draw(P=4096, V=1):
    """nv = 1 at (0.3125, 0.25, 0.25) of the depth-1 tree: a draw stays in the
    leaf (0..0.5 on every axis) unless its x offset exceeds 0.1875, one draw
    in eight, so about 5 % of the paths succeed at exactly the eighth draw --
    the last one the 8-attempt rule allows."""
    nv = np.ones(P, np.int32)
    pos = np.tile(np.asarray(EIGHTH_POS, np.float32), (P, V, 1))
    w = np.ones((P, V, 3), np.float32)
    rec, nv = make_vertices(P, V, nv, pos, w)
    return {"P": P, "V": V, "rec": rec, "nv": nv, "weight": w, "pos": pos}


def first_success(oracle, nodes, pos, leaf_diag, seed, path, d, own_leaf, draws=12):
    """Index of the first jitter draw of vertex d of `path` that finds another
    leaf (None within `draws`), restated from the rule with oracle.rng_uniform
    and oracle.stree_find alone."""
    aabb, child, _ = nodes
    pos = np.asarray(pos, np.float32)
    for k in range(draws):
        u = np.array([oracle.rng_uniform(seed, path, 1024 + d, 3 * k + a) for a in range(3)], np.float32)
        jp = pos + (u - np.float32(0.5)) * np.asarray(leaf_diag, np.float32)
        nb = int(oracle.stree_find(aabb, child, jp[None, :])[0])
        if nb >= 0 and not (aabb[nb, :3] == aabb[own_leaf, :3]).all():
            return k
    return None


SIGMA = np.array([1e-1, 3e-2, 1e-2, 3e-3, 1e-3, 3e-4, 1e-4, 1e-4])


def _clustered(rng, shape):
    """Points around 8 fixed centres with spreads from 1e-1 down to 1e-4."""
    centres = np.random.default_rng(1234).uniform(0.2, 0.8, size=(8, 3))
    k = rng.integers(0, 8, size=shape)
    p = centres[k] + rng.normal(size=shape + (3,)) * SIGMA[k][..., None]
    return np.clip(p, 0.0, 1.0).astype(np.float32)


def deep_tree(oracle, seed=5, n=6000, threshold=24):
    p = _clustered(np.random.default_rng(seed), (n,))
    return oracle.stree_build(LO, HI, 1, [p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()], threshold)


def deep(P=500, seed=6, V=5):
    """Vertices from deep_tree's clusters."""
    rng = np.random.default_rng(seed)
    pos = _clustered(rng, (P, V))
    nv = rng.integers(0, V + 1, size=P).astype(np.int32)
    w = rng.exponential(1.0, size=(P, V, 3)).astype(np.float32)
    w[rng.uniform(size=(P, V)) < 0.15] = 3000.0
    rec, nv = make_vertices(P, V, nv, pos, w, _directions(rng, (P, V)), _directions(rng, (P, V)))
    return {"P": P, "V": V, "rec": rec, "nv": nv, "weight": w, "pos": pos}


def family(oracle, name, P=None):
    """(case, tree nodes) of a named family; `mixed` takes its tree depth from
    the name (mixed1, mixed2)."""
    kw = {} if P is None else {"P": P}
    if name in ("mixed1", "mixed2"):
        return mixed(**kw), unit_tree(oracle, int(name[-1]))
    if name == "single_leaf":
        return single_leaf(**kw), unit_tree(oracle, 0)
    if name == "corner":
        return corner(**kw), unit_tree(oracle, 1)
    if name == "eighth_draw":
        return eighth_draw(**kw), unit_tree(oracle, 1)
    if name == "deep":
        return deep(**kw), deep_tree(oracle)
    raise KeyError(name)


FAMILIES = ("mixed1", "mixed2", "single_leaf", "corner", "eighth_draw", "deep")


def reference(oracle, case, nodes, saved, seed, path0=0):
    """oracle.push_training in (path, push) order, and stably sorted by leaf
    (the order sdmm_push_training returns)."""
    aabb, child, _ = nodes
    ref = oracle.push_training(aabb, child, case["rec"], case["nv"], case["V"], path0, saved, seed)
    order = np.argsort(ref["node"], kind="stable")
    return ref, order
