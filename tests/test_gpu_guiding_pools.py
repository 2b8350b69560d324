"""GPU: the guiding model's pools (guiding.hip: pool_keys / gather / seg /
relabel / count kernels, stats_append, init_gather, order_pool, redistribute,
grow_pool) on constructed vertices, against the reference schedule
(guiding_host_loop.HostLoop fed by oracle.push_training), bitwise after every
optimize: the node arrays, which nodes hold a mixture, every mixture's
parameters and EM state, and the optimize statistics.

All paths have one vertex (nv = 1) on the 1/64 lattice of the unit cube, whose
tree starts as 8 octants (split_depth 1).  Two kinds of position steer the
counts exactly:

  quiet   the quarter of an octant at the tree's outer corner: every jitter
          draw lands in the same octant or outside the tree, so a path gives
          exactly one record (its own leaf's, with a stats entry)
  loud    the quarter at the tree's centre: most draws find a neighbour, whose
          copy's stored point lies outside that neighbour

Each case asserts from the host loop's own tables (HostLoop.log) that the
situation it is named for occurred.
"""
import numpy as np
import pytest

import vertex_cases as vc
from guiding_host_loop import HostLoop, assert_same_mixtures, from_oracle

pytestmark = pytest.mark.gpu

BIG = 1 << 30          # a split threshold no leaf reaches


def _bits(o):
    return [(o >> a) & 1 for a in range(3)]


def quiet(rng, o, n):
    k = np.stack([rng.integers(48, 64, n) if b else rng.integers(1, 17, n) for b in _bits(o)], 1)
    return (k / 64.0).astype(np.float32)


def loud(rng, o, n):
    k = np.stack([rng.integers(33, 40, n) if b else rng.integers(25, 32, n) for b in _bits(o)], 1)
    return (k / 64.0).astype(np.float32)


def quiet_symmetric(rng, o, n):
    """Quiet positions whose x are mirrored about the lattice plane in the
    middle of the quiet cube (and vary most along x): the leaf's split plane is
    exactly that lattice plane, and the positions with x on it lie in both
    children's boxes."""
    b = _bits(o)
    mid = 56 if b[0] else 8
    half = rng.integers(1, 8, n // 2)
    kx = np.concatenate([mid + half, mid - half, np.full(n - 2 * (n // 2), mid)])
    kx[:6] = mid                                   # (a few more on the plane itself; the mean stays there:
    kx[n // 2:n // 2 + 6] = mid                    #  their mirror images too)
    cols = [kx]
    for a in (1, 2):
        c = 56 if b[a] else 8
        cols.append(c + rng.integers(-2, 3, n))
    return (np.stack(cols, 1) / 64.0).astype(np.float32)


def paths(rng, pos, weight=None):
    P = pos.shape[0]
    w = rng.exponential(1.0, size=(P, 1, 3)).astype(np.float32) + np.float32(0.25) if weight is None else weight
    rec, nv = vc.make_vertices(P, 1, np.ones(P, np.int32), pos.reshape(P, 1, 3), w,
                               vc._directions(rng, (P, 1)), vc._directions(rng, (P, 1)))
    return rec, nv


class Pair:
    """The model and the host loop side by side, under one configuration."""

    def __init__(self, pkg, oracle, gpu, K=16, split_depth=1, split_threshold=200, max_leaf_nodes=2048,
                 saved_per_path=8, init_seed=0x1A17, optimize_async=0):
        self.pkg, self.oracle, self.gpu = pkg, oracle, gpu
        self.g = pkg.Guiding(vc.LO, vc.HI, K=K, split_depth=split_depth, split_threshold=split_threshold,
                             max_leaf_nodes=max_leaf_nodes, saved_per_path=saved_per_path, init_seed=init_seed,
                             optimize_async=optimize_async)
        self.tree = pkg.STree(vc.LO, vc.HI)
        self.tree.split_to_depth(split_depth)
        self.loop = HostLoop(pkg, oracle, self.tree, K=K, split_threshold=split_threshold,
                             max_leaf_nodes=max_leaf_nodes, init_seed=init_seed, async_=bool(optimize_async),
                             device=gpu)
        self.saved = saved_per_path

    def leaf(self, p):
        aabb, child, _ = self.tree.nodes()
        return int(self.oracle.stree_find(aabb, child, np.asarray([p], np.float32))[0])

    def octant(self, o):
        return self.leaf([0.25 + 0.5 * b for b in _bits(o)])

    def push(self, rec, nv, seed, path0=0):
        verts = vc.device_vertices(self.pkg, rec, nv, 1, path0, self.gpu)
        self.g.push(verts, seed)
        r = from_oracle(self.oracle, self.tree.nodes(), rec, nv, 1, path0, self.saved, seed)
        self.loop.push(r)
        self.g.update()
        self.loop.update()
        return r

    def compare(self):
        import torch
        torch.cuda.synchronize()
        for a, b in zip(self.tree.nodes(), self.g.tree.nodes()):
            np.testing.assert_array_equal(a, b)
        n = assert_same_mixtures(self.loop.table(), self.g.node_mixtures())
        assert n == self.g.trained
        return n

    def optimize(self, spp):
        got = self.g.optimize(spp)
        want = self.loop.optimize(spp)
        assert got == want, (got, want)
        self.compare()
        return self.loop.log[-1]

    def finish(self):
        """async: the EM the last optimize launched, applied on both sides."""
        self.g.update()
        self.loop.update()
        return self.compare()


def _rng(seed):
    return np.random.default_rng(seed)


# ---------------------------------------------------------------------------

@pytest.mark.parametrize("async_", [0, 1], ids=["sync", "async"])
def test_split_threshold(pkg, oracle, gpu, async_):
    """A leaf at exactly split_threshold stats stays; one more splits -- at a
    lattice plane that holds some of its positions."""
    rng = _rng(1)
    pr = Pair(pkg, oracle, gpu, split_threshold=200, optimize_async=async_)
    A, B = pr.octant(0), pr.octant(7)
    pos = np.concatenate([quiet_symmetric(rng, 0, 200), quiet_symmetric(rng, 7, 201), quiet(rng, 3, 50)])
    pr.push(*paths(rng, pos), seed=11)
    e = pr.optimize(13)
    assert e["n_stats_before"][A] == 200 and e["n_stats_before"][B] == 201
    assert e["over_threshold"] == [B] and e["split"] == [B]
    aabb, child, axis = pr.tree.nodes()
    assert child[A, 0] < 0 and child[B, 0] >= 0
    c0, c1 = child[B]
    assert aabb[c0, 0] == np.float32(56 / 64) == aabb[c1, 3]          # the plane is the lattice plane x = 56/64
    on_plane = int((pos[200:401, 0] == np.float32(56 / 64)).sum())
    assert on_plane >= 6
    # the positions on the plane went to one child only (find: child 0 first)
    assert e["n_stats"][int(c0)] + e["n_stats"][int(c1)] == 201
    # second pass: total_spp = 13 > 12, every leaf with 64 stats and 8 records trains; A, still
    # at the threshold, among them
    pos = np.concatenate([quiet_symmetric(rng, 7, 120), loud(rng, 3, 40)])
    pr.push(*paths(rng, pos), seed=12, path0=(1 << 40) + 5)
    e = pr.optimize(1)
    assert e["split"] == [] and A in e["ready"] and len(e["ready"]) >= 2 and e["fresh"] == e["ready"]
    # one more path: the trained leaf A is over the threshold and splits
    pos = np.concatenate([quiet(rng, 0, 1), quiet_symmetric(rng, 7, 120)])
    pr.push(*paths(rng, pos), seed=13)
    e = pr.optimize(1)
    assert e["n_stats_before"][A] == 201 and A in e["split"] and len([c for v, c in e["inherited"] if v == A]) == 2
    assert e["ready"] and e["fresh"] == []
    assert pr.finish() >= 2


def test_leaf_cap(pkg, oracle, gpu):
    """max_leaf_nodes = the initial leaf count: the first optimize may split
    (<= holds); afterwards a leaf far over the threshold must not."""
    rng = _rng(2)
    pr = Pair(pkg, oracle, gpu, split_threshold=200, max_leaf_nodes=8)
    A, B = pr.octant(1), pr.octant(6)
    pr.push(*paths(rng, quiet(rng, 6, 300)), seed=21)
    e = pr.optimize(1)
    assert not e["capped"] and e["split"] == [B] and pr.tree.leaf_nodes > 8
    nodes_before = pr.tree.num_nodes
    pr.push(*paths(rng, quiet(rng, 1, 1500)), seed=22)
    e = pr.optimize(1)
    assert e["capped"] and e["n_stats_before"][A] == 1500 > 200 and e["split"] == []
    assert pr.tree.num_nodes == nodes_before == pr.g.tree.num_nodes
    assert A in e["ready"]                        # (n_data = 1500 > 1000: trained in place, unsplit)


@pytest.mark.parametrize("async_", [0, 1], ids=["sync", "async"])
def test_ready_rules(pkg, oracle, gpu, async_):
    """Either side of every canBeOptimized comparison."""
    rng = _rng(3)
    pr = Pair(pkg, oracle, gpu, split_threshold=BIG, optimize_async=async_)
    L = [pr.octant(o) for o in range(8)]
    # total_spp = 0: only n_data > 1000 opens the gate
    pos = np.concatenate([quiet(rng, 0, 1000), quiet(rng, 1, 1001), quiet(rng, 2, 63), quiet(rng, 3, 64),
                          quiet(rng, 4, 100)])
    pr.push(*paths(rng, pos), seed=31)
    e = pr.optimize(12)
    assert e["total_spp"] == 0 and e["n_data"][L[0]] == 1000 and e["n_data"][L[1]] == 1001
    assert e["ready"] == [L[1]]
    # total_spp = 12: still not > 12
    e = pr.optimize(1)
    assert e["total_spp"] == 12 and e["ready"] == [] and e["n_data"][L[4]] == 100 and e["n_stats"][L[4]] == 100
    # total_spp = 13: the gate is open; n_stats 63 against 64
    e = pr.optimize(1)
    assert e["total_spp"] == 13 and e["n_stats"][L[2]] == 63 and e["n_stats"][L[3]] == 64
    assert e["ready"] == sorted([L[0], L[3], L[4]])
    # trained leaves (their stats stay, their data is gone): 7 new records against 8
    pos = np.concatenate([quiet(rng, 0, 7), quiet(rng, 4, 8)])
    pr.push(*paths(rng, pos), seed=32)
    e = pr.optimize(1)
    assert e["n_data"][L[0]] == 7 and e["n_data"][L[4]] == 8 and e["n_stats"][L[0]] == 1007
    assert e["ready"] == [L[4]] and e["fresh"] == []
    # the 63-stats leaf with one more path
    pr.push(*paths(rng, quiet(rng, 2, 1)), seed=33)
    e = pr.optimize(1)
    assert e["n_stats"][L[2]] == 64 and e["ready"] == [L[2]] and e["fresh"] == [L[2]]
    assert pr.finish() == 5


def test_iterations_schedule(pkg, oracle, gpu):
    """One leaf optimised six times: 2, 2, 1, 1, ... EM iterations."""
    rng = _rng(4)
    pr = Pair(pkg, oracle, gpu, split_threshold=BIG)
    A = pr.octant(5)
    its, run_ref, run_got = [], [], []
    for r in range(6):
        pos = np.concatenate([quiet(rng, 5, 150), loud(rng, 5, 50)])
        pr.push(*paths(rng, pos), seed=40 + r)
        e = pr.optimize(13)
        if A in e["ready"]:
            its.append(e["iterations"][e["ready"].index(A)])
            run_ref.append(int(pr.loop.mix[A].get_state()["scalars"][3]))
            run_got.append(int(pr.g.node_mixtures()[A].get_state()["scalars"][3]))
    assert its == [2, 2, 1, 1, 1]                  # (the first pass: total_spp = 0 and 200 records)
    assert run_ref == run_got == [2, 4, 5, 6, 7]


@pytest.mark.parametrize("async_", [0, 1], ids=["sync", "async"])
def test_split_of_a_trained_leaf(pkg, oracle, gpu, async_):
    """Every new leaf starts from the parent's mixture and EM state, bitwise --
    also the new leaf that receives no record."""
    rng = _rng(5)
    pr = Pair(pkg, oracle, gpu, split_threshold=2000, optimize_async=async_)
    A = pr.octant(0)
    pr.push(*paths(rng, quiet(rng, 0, 1500)), seed=51)
    e = pr.optimize(0)
    assert e["ready"] == [A] and e["split"] == []
    pr.finish()
    parent = pr.g.node_mixtures()[A]
    pp, ps = parent.get_params(), parent.get_state()
    # 600 more, all at the far end of x: over the threshold, and every record on one side of the plane
    far = quiet(rng, 0, 600)
    far[:, 0] = np.float32(16 / 64)
    pr.push(*paths(rng, far), seed=52)
    e = pr.optimize(0)
    assert e["split"] == [A] and e["ready"] == [] and e["total_spp"] == 0
    new = [c for v, c in e["inherited"] if v == A]
    assert len(new) >= 2
    empty = [c for c in new if e["n_data"].get(c, 0) == 0]
    assert empty, "a new leaf without a record"
    for tab in (pr.g.node_mixtures(), pr.loop.table()):
        assert tab[A] is None
        for c in new:
            cp, cs = tab[c].get_params(), tab[c].get_state()
            for k in ("weights", "mean", "cov", "cholLInv", "detInv", "cdf"):
                np.testing.assert_array_equal(cp[k], pp[k], err_msg=f"leaf {c} {k}")
            for k in ps:
                np.testing.assert_array_equal(cs[k], ps[k], err_msg=f"leaf {c} state {k}")
    # and they train on from there
    pr.push(*paths(rng, quiet(rng, 0, 1200)), seed=53)
    e = pr.optimize(13)
    assert e["ready"] and e["fresh"] == []
    pr.finish()


def test_jitter_copies_dropped_at_a_split(pkg, oracle, gpu):
    """A copy's stored point is the vertex's own, outside the neighbour that
    got the copy: when that neighbour splits, its copies are dropped."""
    rng = _rng(6)
    pr = Pair(pkg, oracle, gpu, split_threshold=200)
    A = pr.octant(0)
    pos = np.concatenate([quiet_symmetric(rng, 0, 150), loud(rng, 1, 190), loud(rng, 2, 190)])
    r = pr.push(*paths(rng, pos), seed=61)
    copies_in_A = int(((r["node"] == A) & ~r["stats"]).sum())
    assert copies_in_A > 20
    e = pr.optimize(1)
    assert e["split"] == [] and e["dropped"] == 0
    pr.push(*paths(rng, quiet_symmetric(rng, 0, 100)), seed=62)
    e = pr.optimize(1)
    assert A in e["split"] and e["dropped"] >= copies_in_A and e["dropped_stats"] == 0
    assert e["stats"]["records"] == sum(e["n_data"].values())
    pr.push(*paths(rng, np.concatenate([quiet(rng, 0, 300), loud(rng, 1, 100)])), seed=63)
    e = pr.optimize(13)
    e = pr.optimize(1)
    assert e["total_spp"] > 12 and e["ready"]


def test_pool_regrowth_with_live_contents(pkg, oracle, gpu):
    """A few hundred records, then more than 65536 into the live pool (the
    first pool holds 65536): nothing is lost or reordered -- the leaves'
    initial K/8 records and their EM sums depend on the order."""
    rng = _rng(7)
    pr = Pair(pkg, oracle, gpu, split_threshold=BIG)
    pos = np.concatenate([quiet(rng, o, 40) for o in range(8)] + [loud(rng, 0, 30)])
    r0 = pr.push(*paths(rng, pos), seed=71)
    assert 300 < r0["node"].shape[0] < 1000
    pos = np.concatenate([quiet(rng, o, 8200) for o in range(8)] + [loud(rng, o, 300) for o in range(8)])
    r1 = pr.push(*paths(rng, pos), seed=72, path0=(1 << 40) + 5)
    assert r1["node"].shape[0] > 65536
    e = pr.optimize(1)
    assert e["stats"]["records"] == r0["node"].shape[0] + r1["node"].shape[0]
    assert len(e["ready"]) == 8 == len(e["fresh"])
    # the first push's records lead every leaf's data: they seeded the leaves
    for v in e["ready"]:
        assert (r0["node"] == v).sum() >= 2


def test_many_nodes(pkg, oracle, gpu):
    """65535 nodes (over the count kernel's LDS bins, 17-bit sort keys), the
    default leaf cap (so nothing splits), a few thousand vertices in a handful
    of leaves."""
    rng = _rng(8)
    pr = Pair(pkg, oracle, gpu, split_depth=5, split_threshold=200)
    assert pr.tree.num_nodes == 65535 == pr.g.tree.num_nodes
    cells = np.array([[0, 0, 0], [31, 31, 31], [16, 15, 16], [16, 16, 16], [5, 20, 9], [31, 0, 17]])
    pos = []
    for c, n in zip(cells, (1200, 1100, 900, 700, 300, 60)):
        u = rng.uniform(0.05, 0.95, size=(n, 3))
        pos.append(((c + u) / 32.0).astype(np.float32))
    on_planes = (cells[2:4, None, :] + rng.integers(0, 3, size=(2, 200, 3)) / 2.0).reshape(-1, 3) / 32.0
    pos = np.concatenate(pos + [on_planes.astype(np.float32)])
    r = pr.push(*paths(rng, pos), seed=81)
    assert np.unique(r["node"]).size > 6 and r["node"].max() > 16384
    e = pr.optimize(13)
    assert e["capped"] and max(e["n_stats_before"].values()) > 200
    assert len(e["ready"]) >= 2 and max(e["ready"]) > 16384
    pr.push(*paths(rng, pos[::3].copy()), seed=82)
    e = pr.optimize(1)
    assert len(e["ready"]) >= 4 and e["fresh"] and set(e["ready"]) - set(e["fresh"])
    assert pr.tree.num_nodes == 65535


def test_push_that_yields_nothing(pkg, oracle, gpu):
    """Vertices all lost or with a non-finite weight: the push and an optimize
    on empty pools are no-ops."""
    rng = _rng(9)
    pr = Pair(pkg, oracle, gpu, split_threshold=BIG)
    P = 500
    pos = quiet(rng, 0, P)
    pos[:200, 0] = 1.5
    pos[200:250, 1] = np.nan
    w = np.ones((P, 1, 3), np.float32)
    w[250:400, 0, 1] = np.nan
    w[400:, 0, 2] = np.inf
    rec, nv = paths(rng, pos, weight=w)
    e0 = pr.optimize(1)                            # before any push
    r = pr.push(rec, nv, seed=91)
    assert r["node"].shape[0] == 0 and r["lost"] == 250
    e = pr.optimize(1)
    assert e["stats"] == e0["stats"] == {"leaves": 8, "optimized": 0, "records": 0}
    assert pr.g.trained == 0
    # and the model still works afterwards
    pr.push(*paths(rng, quiet(rng, 0, 1100)), seed=92)
    e = pr.optimize(1)
    assert len(e["ready"]) == 1


def test_wider_mixtures(pkg, oracle, gpu):
    """K = 128: several fresh leaves at once, each initialised from its first
    K/8 = 16 records (init_gather_kernel)."""
    rng = _rng(10)
    pr = Pair(pkg, oracle, gpu, K=128, split_threshold=BIG)
    pos = np.concatenate([quiet(rng, o, 1100) for o in (0, 3, 5, 6)] + [loud(rng, o, 200) for o in (1, 2)])
    pr.push(*paths(rng, pos), seed=101)
    e = pr.optimize(1)
    assert len(e["fresh"]) == 4 == len(e["ready"])
    pr.push(*paths(rng, np.concatenate([quiet(rng, o, 1100) for o in (0, 3, 7)])), seed=102)
    e = pr.optimize(1)
    assert len(e["ready"]) == 3 and len(e["fresh"]) == 1
