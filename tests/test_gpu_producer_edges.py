"""GPU: the training-data producer (produce_count / write / gather / seg
kernels, push_training_ex) on constructed vertices (vertex_cases.py) against
the host-routed reference (oracle.push_training), exactly: vertices outside
the tree and at NaN positions, non-finite and overflowing average weights,
the > 1000 second jitter copy and its boundary, the 8-attempt rule, nv = 0,
saved_per_path on either side of nv and max_vertices, a 64-bit path0, P on
either side of a 256-thread block, and the API's count-only, capacity and
nullable-plane paths.  test_vertex_cases.py shows on the oracle alone that
each family reaches its branch."""
import ctypes as C

import numpy as np
import pytest

import vertex_cases as vc
from producer_check import check_records

pytestmark = pytest.mark.gpu

SEED = 0x5EED
BIG_PATH0 = (1 << 40) + 5
SENTINEL = -12345.0


def _run(pkg, oracle, gpu, case, nodes, saved, seed, path0, tag, plog=None):
    import torch
    tree = vc.device_tree(pkg, nodes)
    verts = vc.device_vertices(pkg, case["rec"], case["nv"], case["V"], path0, gpu)
    out = tree.push_training(verts, saved, seed)
    torch.cuda.synchronize()
    ref = oracle.push_training(nodes[0], nodes[1], case["rec"], case["nv"], case["V"], path0, saved, seed)
    check_records(out, ref, case["rec"], case["nv"], case["V"], tree.num_nodes, tag, plog)
    return out, ref


_CASES = [(name, saved, (0, BIG_PATH0)[(i + j) % 2])
          for i, name in enumerate(vc.FAMILIES) for j, saved in enumerate((1, 3, 8, 20))]


@pytest.mark.parametrize("name,saved,path0", _CASES, ids=lambda v: str(v))
def test_family_matches_host_reference(pkg, oracle, gpu, plog, name, saved, path0):
    case, nodes = vc.family(oracle, name)
    out, ref = _run(pkg, oracle, gpu, case, nodes, saved, SEED, path0, f"{name}_s{saved}", plog)
    assert ref["node"].shape[0] > 0
    if name.startswith("mixed") or name == "single_leaf":
        assert out["lost"] > 0
    if name in ("mixed1", "mixed2", "deep") and saved >= 3:
        V = case["V"]
        src, st = out["source"].cpu().numpy(), out["stats"].cpu().numpy()
        assert ((st == 0) & (src % V < case["nv"][src // V] - 1)).any()    # the > 1000 copy of an inner vertex


def test_path0_enters_the_draws(pkg, oracle, gpu):
    """The same vertices under path0 = 0 and 2^40 + 5 jitter differently (and
    each equals its reference): the high word of path0 is not dropped."""
    case, nodes = vc.family(oracle, "mixed2")
    a, _ = _run(pkg, oracle, gpu, case, nodes, 8, SEED, 0, "p0")
    b, _ = _run(pkg, oracle, gpu, case, nodes, 8, SEED, BIG_PATH0, "p40")
    c, _ = _run(pkg, oracle, gpu, case, nodes, 8, SEED, 5, "p5")
    assert not np.array_equal(a["seg"], b["seg"]) and not np.array_equal(c["seg"], b["seg"])


@pytest.mark.parametrize("P", [1, 255, 256, 257, 4099])
@pytest.mark.parametrize("name", ["mixed2", "deep"])
def test_block_edges(pkg, oracle, gpu, name, P):
    case, nodes = vc.family(oracle, name, P=P)
    if P == 1:
        case["nv"][:] = case["V"]           # the one path visits every vertex
    _run(pkg, oracle, gpu, case, nodes, 8, SEED + P, BIG_PATH0 if P % 2 else 0, f"{name}_P{P}")


@pytest.mark.parametrize("P", [1, 257])
def test_no_vertices(pkg, oracle, gpu, P):
    case, nodes = vc.family(oracle, "mixed2", P=P)
    case["nv"][:] = 0
    out, ref = _run(pkg, oracle, gpu, case, nodes, 8, SEED, 0, f"nv0_P{P}")
    assert out["w"].numel() == 0 and (out["seg"] == 0).all() and out["lost"] == 0


def test_no_paths(pkg, oracle, gpu):
    nodes = vc.unit_tree(oracle, 2)
    tree = vc.device_tree(pkg, nodes)
    rec, nv = vc.make_vertices(0, 9, np.zeros(0, np.int32), np.zeros((0, 9, 3)), np.zeros((0, 9, 3)))
    verts = vc.device_vertices(pkg, rec, nv, 9, 0, gpu)
    out = tree.push_training(verts, 8, SEED)
    assert out["w"].numel() == 0 and out["seg"].shape == (tree.num_nodes + 1,) and (out["seg"] == 0).all()
    assert out["lost"] == 0


# ---- the C ABI's own paths (count only, capacity, nullable planes)

_PLANES = [f"x{i}" for i in range(6)] + [f"normal{i}" for i in range(3)] + ["w", "stats", "node", "source"]


def _buffers(gpu, m):
    import torch
    b = {}
    for k in _PLANES:
        dt = {"stats": torch.uint8, "node": torch.int32, "source": torch.int64}.get(k, torch.float32)
        b[k] = torch.full((m,), 77 if dt != torch.float32 else SENTINEL, dtype=dt, device=gpu)
    return b


def _raw(pkg, tree, verts, saved, seed, bufs, capacity, null=(), want_seg=True, want_lost=True):
    """sdmm_push_training itself -> (rc, n_out, seg, lost); bufs None: count only."""
    import torch
    n, lost = C.c_int64(-1), C.c_int64(-7)
    seg = np.full(tree.num_nodes + 1, -1, np.int64)
    o = None
    if bufs is not None:
        o = pkg._TrainingOut()
        ptr = lambda k: None if k in null else bufs[k].data_ptr()
        for i in range(6):
            o.x[i] = ptr(f"x{i}")
        for i in range(3):
            o.normal[i] = ptr(f"normal{i}")
        o.w, o.stats, o.node, o.source = ptr("w"), ptr("stats"), ptr("node"), ptr("source")
        o.capacity = capacity
    rc = pkg.lib().sdmm_push_training(tree.h, C.byref(verts.s), int(saved), C.c_uint64(seed),
                                      None if o is None else C.byref(o), C.byref(n),
                                      seg.ctypes.data_as(C.c_void_p) if want_seg else None,
                                      C.byref(lost) if want_lost else None)
    torch.cuda.synchronize()
    return rc, n.value, seg, lost.value


@pytest.fixture(scope="module")
def api_case(pkg, oracle, gpu):
    case, nodes = vc.family(oracle, "mixed2")
    tree = vc.device_tree(pkg, nodes)
    verts = vc.device_vertices(pkg, case["rec"], case["nv"], case["V"], BIG_PATH0, gpu)
    ref = oracle.push_training(nodes[0], nodes[1], case["rec"], case["nv"], case["V"], BIG_PATH0, 8, SEED)
    assert ref["lost"] > 0 and ref["node"].shape[0] > 1000
    return case, nodes, tree, verts, ref


def test_count_only_call(pkg, gpu, api_case):
    """out NULL: *n_out is the writing call's count; seg is left alone and
    *lost is 0 -- lost is reported by a writing call only (sdmm_gpu.h)."""
    case, nodes, tree, verts, ref = api_case
    m = ref["node"].shape[0]
    rc, n, seg, lost = _raw(pkg, tree, verts, 8, SEED, None, 0)
    assert rc == 0 and n == m
    assert (seg == -1).all() and lost == 0
    bufs = _buffers(gpu, m)
    rc, n2, seg, lost = _raw(pkg, tree, verts, 8, SEED, bufs, m)
    assert rc == 0 and n2 == n and lost == ref["lost"] > 0
    np.testing.assert_array_equal(seg, np.concatenate([[0], np.cumsum(np.bincount(ref["node"], minlength=tree.num_nodes))]))


def test_capacity_one_short_writes_nothing(pkg, gpu, api_case):
    case, nodes, tree, verts, ref = api_case
    m = ref["node"].shape[0]
    bufs = _buffers(gpu, m)
    rc, n, seg, lost = _raw(pkg, tree, verts, 8, SEED, bufs, m - 1)
    assert rc == -1        # SDMM_E_INVALID
    assert n == m
    want = _buffers(gpu, m)
    import torch
    for k in _PLANES:
        assert torch.equal(bufs[k], want[k]), k
    assert (seg == -1).all() and lost == 0


@pytest.mark.parametrize("null", [("normal0", "normal1", "normal2"), ("stats",), ("node",), ("source",),
                                  ("normal0", "normal1", "normal2", "stats", "node", "source")],
                         ids=["normal", "stats", "node", "source", "all"])
@pytest.mark.parametrize("host_out", [True, False], ids=["seg_lost", "no_seg_lost"])
def test_nullable_planes(pkg, gpu, api_case, null, host_out):
    """A null optional plane (and null seg / lost) changes nothing in the
    planes that remain, and the null plane's buffer is not written."""
    import torch
    case, nodes, tree, verts, ref = api_case
    m = ref["node"].shape[0]
    full = _buffers(gpu, m)
    rc, n, seg0, lost0 = _raw(pkg, tree, verts, 8, SEED, full, m)
    assert rc == 0 and n == m
    bufs = _buffers(gpu, m)
    rc, n, seg, lost = _raw(pkg, tree, verts, 8, SEED, bufs, m, null=null, want_seg=host_out, want_lost=host_out)
    assert rc == 0 and n == m
    untouched = _buffers(gpu, m)
    for k in _PLANES:
        assert torch.equal(bufs[k], untouched[k] if k in null else full[k]), k
    if host_out:
        np.testing.assert_array_equal(seg, seg0)
        assert lost == lost0 == ref["lost"]
    else:
        assert (seg == -1).all() and lost == -7


def test_host_side_rejections(pkg, gpu, api_case):
    """Only what the host rejects before any launch: saved < 1, n_out NULL, a
    negative path count, max_vertices < 1."""
    case, nodes, tree, verts, ref = api_case
    m = ref["node"].shape[0]
    bufs = _buffers(gpu, m)
    rc, n, _, _ = _raw(pkg, tree, verts, 0, SEED, bufs, m)
    assert rc == -1
    s = pkg._PathVertices()
    s.n_paths, s.max_vertices, s.path0, s.rec, s.nv = -1, 9, 0, verts.s.rec, verts.s.nv
    bad = pkg.PathVertices(s, None, 0)
    assert _raw(pkg, tree, bad, 8, SEED, bufs, m)[0] == -1
    s.n_paths, s.max_vertices = verts.s.n_paths, 0
    assert _raw(pkg, tree, bad, 8, SEED, bufs, m)[0] == -1
    rc = pkg.lib().sdmm_push_training(tree.h, C.byref(verts.s), 8, C.c_uint64(SEED), None, None, None, None)
    assert rc == -1
    untouched = _buffers(gpu, m)
    import torch
    for k in _PLANES:
        assert torch.equal(bufs[k], untouched[k]), k


@pytest.mark.parametrize("name,depth", [("single_leaf", 0), ("mixed1", 1), ("mixed2", 2)])
def test_guiding_push_reuses_the_count(pkg, oracle, gpu, name, depth):
    """sdmm_guiding_push: a count-only call, then the write with the count
    pass's offsets reused (reuse_counts).  The pool then holds exactly the
    reference's records -- their number here; their contents are pinned by the
    bitwise training of test_gpu_guiding_pools.py."""
    case, nodes = vc.family(oracle, name, P=200)      # (few enough records that no leaf can be optimised)
    g = pkg.Guiding(vc.LO, vc.HI, split_depth=depth, split_threshold=1 << 30, saved_per_path=3)
    for a, b in zip(nodes, g.tree.nodes()):
        np.testing.assert_array_equal(a, b)
    verts = vc.device_vertices(pkg, case["rec"], case["nv"], case["V"], BIG_PATH0, gpu)
    total = 0
    for it in range(2):
        g.push(verts, SEED + it)
        total += oracle.push_training(nodes[0], nodes[1], case["rec"], case["nv"], case["V"], BIG_PATH0, 3,
                                      SEED + it)["node"].shape[0]
        # the tree's own producer call between two pushes must not disturb the next one
        g.tree.push_training(verts, 8, SEED)
    st = g.optimize(0)
    assert st["records"] == total > 0 and st["leaves"] == 8 ** depth and st["optimized"] == 0
