"""The constructed vertex families (vertex_cases.py) on the CPU oracle alone:
every family reaches the branch of the training-data producer it was built
for, so no test of test_gpu_producer_edges.py / test_gpu_guiding_pools.py can
pass vacuously.  A family that stops reaching its branch fails here, without
a GPU."""
import numpy as np
import pytest

import vertex_cases as vc

SEED = 0x5EED


def _split(case, ref):
    V = case["V"]
    p, d = ref["source"] // V, ref["source"] % V
    jit = ref["stats"] == 0
    return p, d, jit, jit & (d < case["nv"][p] - 1)


def _found(pos):
    with np.errstate(invalid="ignore"):
        return ((pos >= 0.0) & (pos <= 1.0)).all(-1)


def test_boundary_triples_are_what_they_claim():
    t0, t1 = vc.boundary_triples()
    assert vc.average(t0) == np.float32(1000.0)
    assert vc.average(t1) > np.float32(1000.0)
    # the inputs are adjacent: no float32 sum lies between the two triples'
    assert (t1[0] + t1[1]) + t1[2] == np.nextafter(np.float32(3000.0), np.float32(np.inf))


@pytest.mark.parametrize("name", ["mixed1", "mixed2"])
@pytest.mark.parametrize("saved", [3, 8, 20])
def test_mixed_reaches_every_class(oracle, name, saved):
    case, nodes = vc.family(oracle, name)
    ref, _ = vc.reference(oracle, case, nodes, saved, SEED)
    p, d, jit, jit_inner = _split(case, ref)
    vis = vc.visited(case["nv"], case["V"], saved)
    for cname, c in vc.WEIGHT_CLASSES.items():
        assert (vis & (case["weight_class"] == c)).sum() >= 3, cname
    for cname, c in vc.POSITION_CLASSES.items():
        assert (vis & (case["position_class"] == c)).sum() >= 3, cname
    # nv covers 0, V and what lies between; saved on either side of nv
    assert (case["nv"] == 0).any() and (case["nv"] == case["V"]).any()
    assert (case["nv"] > saved).any() or saved >= case["V"]
    # the classes do what they were built for
    avg = vc.average(case["weight"])
    wc = case["weight_class"]
    assert not np.isfinite(avg[wc == vc.W_OVERFLOW]).any() and np.isfinite(case["weight"][wc == vc.W_OVERFLOW]).all()
    assert np.isnan(avg[wc == vc.W_INF_MINUS_INF]).all() and np.isinf(avg[wc == vc.W_INF]).all()
    found = _found(case["pos"])
    assert ref["lost"] == int((vis & ~found).sum()) > 0
    # records: one own-leaf record per found, finite, visited vertex
    assert int((~jit).sum()) == int((vis & found & np.isfinite(avg)).sum())
    # average > 1000 at a vertex that is not the last one: the second jitter copy
    assert 50 <= int(jit_inner.sum()) <= 400
    assert (avg[p[jit_inner], d[jit_inner]] > 1000.0).all()
    # a non-finite weight emits no record at all
    assert np.isfinite(ref["w"]).all()


@pytest.mark.parametrize("saved", [1, 3, 8, 20])
def test_single_leaf_gives_up_every_jitter(oracle, saved):
    case, nodes = vc.family(oracle, "single_leaf")
    assert nodes[0].shape[0] == 1
    ref, _ = vc.reference(oracle, case, nodes, saved, SEED)
    vis = vc.visited(case["nv"], case["V"], saved)
    ok = vis & _found(case["pos"]) & np.isfinite(vc.average(case["weight"]))
    assert int((ref["stats"] == 0).sum()) == 0
    assert ref["node"].shape[0] == int(ok.sum()) > 0
    assert ref["lost"] > 0


def test_corner_draws_never_leave(oracle):
    case, nodes = vc.family(oracle, "corner")
    ref, _ = vc.reference(oracle, case, nodes, 8, SEED)
    assert ref["node"].shape[0] == 4096 == case["P"]
    assert (ref["stats"] == 1).all() and ref["lost"] == 0
    assert np.unique(ref["node"]).size == 1


def test_eighth_draw_is_the_last_allowed(oracle):
    case, nodes = vc.family(oracle, "eighth_draw")
    ref, _ = vc.reference(oracle, case, nodes, 8, SEED)
    aabb, child, _ = nodes
    own = int(oracle.stree_find(aabb, child, np.asarray([vc.EIGHTH_POS], np.float32))[0])
    diag = aabb[own, 3:] - aabb[own, :3]
    first = [vc.first_success(oracle, nodes, vc.EIGHTH_POS, diag, SEED, p, 0, own) for p in range(case["P"])]
    first = np.array([-1 if k is None else k for k in first])
    has_jit = np.zeros(case["P"], bool)
    has_jit[ref["source"][ref["stats"] == 0] // case["V"]] = True
    # a success at draw 0..7 is taken; one that would come at draw 8 or later is not
    np.testing.assert_array_equal(has_jit, (first >= 0) & (first <= 7))
    assert int((first == 7).sum()) >= 50 and int((first >= 8).sum()) >= 50 and int((first < 0).sum()) >= 50
    assert int((ref["stats"] == 1).sum()) == case["P"]


def test_deep_spans_decades_and_jitters(oracle):
    case, nodes = vc.family(oracle, "deep")
    aabb, child, _ = nodes
    leaf = child[:, 0] < 0
    size = (aabb[leaf, 3:] - aabb[leaf, :3]).max(1)
    assert size.max() / size.min() >= 1e3 and leaf.sum() > 100
    ref, _ = vc.reference(oracle, case, nodes, 8, SEED)
    p, d, jit, jit_inner = _split(case, ref)
    assert jit_inner.sum() >= 20 and ref["lost"] == 0
    # records reach small and large leaves alike
    rs = (aabb[ref["node"], 3:] - aabb[ref["node"], :3]).max(1)
    assert rs.max() / rs.min() >= 1e3


@pytest.mark.parametrize("depth", [1, 2])
def test_exactly_1000_adds_no_copy_and_the_next_average_does(oracle, depth):
    """Two builds that differ only in the near-1000 weights: every such vertex
    at exactly 1000.0f, or at the next average above.  > 1000 is strict."""
    nodes = vc.unit_tree(oracle, depth)
    exact, nxt, both = (vc.mixed(boundary=b) for b in ("exact", "next", "both"))
    near = (exact["weight_class"] == vc.W_1000) | (exact["weight_class"] == vc.W_1000_NEXT)
    np.testing.assert_array_equal(exact["weight"][~near].view(np.uint32), nxt["weight"][~near].view(np.uint32))
    r = {}
    for k, case in (("exact", exact), ("next", nxt), ("both", both)):
        ref, _ = vc.reference(oracle, case, nodes, 8, SEED)
        p, d, jit, jit_inner = _split(case, ref)
        r[k] = (ref, case["weight_class"][p, d], jit, jit_inner)
    n_exact, n_next = r["exact"][0]["node"].shape[0], r["next"][0]["node"].shape[0]
    assert n_next > n_exact
    ref, wc, jit, jit_inner = r["exact"]
    assert not (jit_inner & ((wc == vc.W_1000) | (wc == vc.W_1000_NEXT))).any()
    ref, wc, jit, jit_inner = r["next"]
    extra = int((jit_inner & ((wc == vc.W_1000) | (wc == vc.W_1000_NEXT))).sum())
    assert extra > 0
    ref, wc, jit, jit_inner = r["both"]
    assert not (jit_inner & (wc == vc.W_1000)).any() and (jit_inner & (wc == vc.W_1000_NEXT)).any()
    # the second copy of a LAST vertex counts too: the builds differ by every
    # second draw sequence that found another leaf
    assert n_next - n_exact >= extra
