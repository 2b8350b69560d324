"""Triangle meshes on the host (no GPU): sdmm_scene_intersect_host's BVH against
its brute-force loop and against a float64 restatement, the description's
validation, the BVH's shape (sdmm_mesh_bvh_dump) and a sanitizer run of the
build and the traversal as a stand-alone program.  The same on a mesh whose
BVH is as deep as the traversal stack allows (24 inner levels, triangles over
six decades of size), on grazing, surface-leaving, signed-zero and non-finite
rays, on rays through shared vertices and edges, on exact ties, and at the
edge of the scale envelope in which walk == loop holds."""
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import mesh_fixture as mf  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]


def _host(pkg, desc, o, d, mode, mint=mf.MINT, maxt=np.inf):
    return pkg.intersect_host(desc, o, d, mint, maxt, mode)


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def test_bvh_equals_brute_force(pkg, scenes):
    """Mode 0 == mode 1 bitwise on (prim, t) for every ray of the fixture."""
    o, d, kinds = mf.rays(scenes)
    desc = mf.torus_desc(scenes)
    bvh, brute = _host(pkg, desc, o, d, 0), _host(pkg, desc, o, d, 1)
    assert _same(bvh, brute)
    prim, t = bvh
    assert (prim >= 3).mean() > 0.4          # many rays hit the torus (ids n_quads + i)
    assert prim[kinds["miss"]] == -1 and np.isinf(t[kinds["miss"]])
    assert np.all(np.isinf(t[prim < 0])) and np.all(t[prim >= 0] > mf.MINT)
    # maxt just below and just above a known hit
    k = kinds["known_hit"]
    assert prim[k] >= 3
    for mode in (0, 1):
        below = _host(pkg, desc, o[k:k + 1], d[k:k + 1], mode, maxt=np.nextafter(t[k], np.float32(0)))
        above = _host(pkg, desc, o[k:k + 1], d[k:k + 1], mode, maxt=np.nextafter(t[k], np.float32(np.inf)))
        assert above[0][0] == prim[k] and above[1][0] == t[k]
        assert below[0][0] != prim[k]
    assert _same(_host(pkg, desc, o, d, 0, maxt=2.5), _host(pkg, desc, o, d, 1, maxt=2.5))


@pytest.mark.parametrize("which", [0, 1, 2])
def test_bvh_equals_brute_force_small_and_doubled(pkg, scenes, which):
    o, d, _ = mf.rays(scenes)
    name, desc = mf.small_descs(scenes)[which]
    bvh, brute = _host(pkg, desc, o, d, 0), _host(pkg, desc, o, d, 1)
    assert _same(bvh, brute), name
    assert (bvh[0] >= 3).any(), name
    if name == "doubled":
        # the torus lies on itself: every hit reports the lower id, and is the single torus' hit
        single = _host(pkg, mf.torus_desc(scenes), o, d, 0)
        assert bvh[0].max() < 3 + 576
        assert _same(bvh, single)


def _f64_reference(desc, o, d, dtype=np.float64, mint=mf.MINT):
    """Moeller-Trumbore (core/triangle.h:109-145) and the quads' plane test
    restated in numpy at `dtype`: per ray (t [nq, n_prims], inside margin [nq,
    n_prims]) -- t = inf where the primitive is missed; margin: the least
    distance of the barycentrics (quad: of its two coordinates) to an edge.
    A description without quads has the triangles alone."""
    o, d = o.astype(dtype), d.astype(dtype)
    v = desc["mesh_vertices"].reshape(-1, 3).astype(dtype)
    tri = desc["triangles"].reshape(-1, 3)
    p0 = v[tri[:, 0]]
    e1, e2 = v[tri[:, 1]] - p0, v[tri[:, 2]] - p0
    with np.errstate(all="ignore"):
        pvec = np.cross(d[:, None, :], e2[None])
        det = (e1[None] * pvec).sum(-1)
        inv = dtype(1) / det
        tvec = o[:, None, :] - p0[None]
        u = (tvec * pvec).sum(-1) * inv
        qvec = np.cross(tvec, e1[None])
        vv = (d[:, None, :] * qvec).sum(-1) * inv
        t = (e2[None] * qvec).sum(-1) * inv
        ok = (det != 0) & (u >= 0) & (u <= 1) & (vv >= 0) & (u + vv <= 1) & (t > mint)
        margin = np.minimum(np.minimum(u, vv), 1 - u - vv)
        tt = np.where(ok, t, np.inf)
        if "quads" not in desc:
            return tt, margin
        q = desc["quads"].reshape(-1, 3, 3).astype(dtype)
        n = np.cross(q[:, 1], q[:, 2])
        den = d @ n.T
        tq = ((q[None, :, 0] - o[:, None]) * n[None]).sum(-1) / den
        r = o[:, None] + tq[..., None] * d[:, None] - q[None, :, 0]
        g1 = np.cross(q[:, 2], n) / (q[:, 1] * np.cross(q[:, 2], n)).sum(-1, keepdims=True)
        g2 = np.cross(n, q[:, 1]) / (q[:, 2] * np.cross(n, q[:, 1])).sum(-1, keepdims=True)
        a, b = (r * g1[None]).sum(-1), (r * g2[None]).sum(-1)
        okq = (den != 0) & (tq > mint) & (a >= 0) & (a <= 1) & (b >= 0) & (b <= 1)
        mq = np.minimum(np.minimum(a, 1 - a), np.minimum(b, 1 - b))
    return (np.concatenate([np.where(okq, tq, np.inf), tt], 1), np.concatenate([mq, margin], 1))


def test_against_float64(pkg, scenes):
    """The same primitive as a float64 restatement of the formula on every
    ray that is not ambiguous (two smallest float64 t within 1e-5 relative, or
    the winner's barycentric within 1e-5 of an edge), at most 0.5 % ambiguous;
    t within 4x the worst error of a numpy float32 restatement on these rays
    (2.51e-5 relative when this was written, the library's own error the same:
    cancellation for origins 3 units away; the 4x covers operation-order
    differences between numpy and C)."""
    o, d, kinds = mf.rays(scenes)
    o, d = o[kinds["random"]], d[kinds["random"]]        # the aimed and unaimed rays
    desc = mf.torus_desc(scenes)
    prim, t = _host(pkg, desc, o, d, 0)
    t64, m64 = _f64_reference(desc, o, d)
    order = np.argsort(t64, 1)
    rows = np.arange(len(o))
    win = order[:, 0]
    tw, t2 = t64[rows, win], t64[rows, order[:, 1]]
    hit = np.isfinite(tw)
    with np.errstate(invalid="ignore"):
        ambiguous = hit & ((np.isfinite(t2) & (t2 - tw < 1e-5 * tw)) | (m64[rows, win] < 1e-5))
    share = ambiguous.mean()
    print(f"ambiguous rays: {int(ambiguous.sum())} of {len(o)} ({share:.4%})")
    assert share <= 0.005
    ref_prim = np.where(hit, win, -1)
    clear = ~ambiguous
    assert np.array_equal(prim[clear], ref_prim[clear])
    # hit distance on the triangle hits
    sel = clear & hit & (win >= 3)
    t32, _ = _f64_reference(desc, o, d, np.float32)
    t32w = t32[rows, win]
    ok32 = sel & np.isfinite(t32w)
    err32 = float(np.max(np.abs(t32w[ok32].astype(np.float64) - tw[ok32]) / tw[ok32]))
    err = float(np.max(np.abs(t[sel].astype(np.float64) - tw[sel]) / tw[sel]))
    print(f"relative t error: library {err:.3e}, numpy float32 restatement {err32:.3e} (bound 4x = {4 * err32:.3e})")
    assert err32 > 0
    assert err <= 4 * err32


def _expect_invalid(pkg, desc, word):
    with pytest.raises(pkg.SDMMError, match="sdmm error -1") as e:
        pkg.intersect_host(desc, np.zeros((1, 3), np.float32), np.ones((1, 3), np.float32), mf.MINT, np.inf, 0)
    assert word in str(e.value), str(e.value)


def test_validation(pkg, scenes):
    o, d, _ = mf.rays(scenes)
    good = mf.torus_desc(scenes)

    def changed(**kw):
        c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in good.items()}
        c.update(kw)
        return c
    tri = good["triangles"].copy()
    tri[7] = 288                                       # one past the last vertex
    _expect_invalid(pkg, changed(triangles=tri), "index out of range")
    tri[7] = -1
    _expect_invalid(pkg, changed(triangles=tri), "index out of range")
    for bad in (np.nan, np.inf):
        v = good["mesh_vertices"].copy()
        v[100] = bad
        _expect_invalid(pkg, changed(mesh_vertices=v), "non-finite vertex")
    tri = good["triangles"].copy()
    tri[3:6] = [5, 5, 9]                               # two corners coincide
    _expect_invalid(pkg, changed(triangles=tri), "zero-area")
    tri[3:6] = [0, 12, 24]                             # three vertices at one point
    v = good["mesh_vertices"].copy().reshape(-1, 3)
    v[12] = v[0]
    v[24] = v[0]
    _expect_invalid(pkg, changed(triangles=tri, mesh_vertices=v.reshape(-1)), "zero-area")
    tb = good["tri_bsdf"].copy()
    tb[11] = 1
    _expect_invalid(pkg, changed(tri_bsdf=tb), "material index out of range")
    tb[11] = -1
    _expect_invalid(pkg, changed(tri_bsdf=tb), "material index out of range")
    te = np.full(576, -1, np.int32)
    te[5] = 1
    _expect_invalid(pkg, changed(tri_emitter=te, radiance=np.ones(3, np.float32)), "material index out of range")
    te[5] = -2
    _expect_invalid(pkg, changed(tri_emitter=te, radiance=np.ones(3, np.float32)), "material index out of range")
    no_bsdf = changed()
    del no_bsdf["tri_bsdf"]
    _expect_invalid(pkg, no_bsdf, "tri_bsdf")
    # a BVH deeper than the traversal stack: 576 triangles need 8 inner levels
    with pytest.raises(pkg.SDMMError, match="deeper than the traversal stack"):
        pkg.mesh_bvh_dump(good, max_levels=7)
    assert pkg.mesh_bvh_dump(good, max_levels=8)["levels"] == 8
    # n_triangles = 0 with garbage in the other mesh fields: the quad-only answer
    quads_only = {k: good[k] for k in ("quads", "bsdf", "reflectance")}
    ref = _host(pkg, quads_only, o, d, 0)
    assert (ref[0] >= 0).any()
    sd, keep = pkg._SceneDesc(), {}
    pkg._fill_geometry(sd, quads_only, keep)
    sd.n_mesh_vertices, sd.mesh_vertices = -7, 0x10
    sd.triangles, sd.tri_bsdf, sd.tri_emitter, sd.tri_flip_normals = 0x10, 0x20, 0x30, 0x40
    for mode in (0, 1):
        prim, t = np.empty(len(o), np.int32), np.empty(len(o), np.float32)
        pkg._check(pkg.lib().sdmm_scene_intersect_host(
            pkg.C.byref(sd), len(o), o.ctypes.data, d.ctypes.data, mf.MINT, float("inf"), mode, prim.ctypes.data,
            t.ctypes.data))
        assert _same((prim, t), ref)


@pytest.mark.parametrize("cap", [0, 8])
def test_tree_shape(pkg, scenes, cap):
    """Every triangle in exactly one leaf, leaves of at most 4, every child
    box inside its parent's, the depth within the cap.  The deep meshes reach
    the traversal stack's cap, 24 inner levels, exactly."""
    desc = mf.torus_desc(scenes)
    deep = [(which, mf.deep_desc(pkg, which)) for which in mf.DEEP] if cap == 0 else []
    for name, dsc in [("torus", desc)] + (mf.small_descs(scenes) if cap == 0 else []) + deep:
        T = pkg.mesh_bvh_dump(dsc, max_levels=cap)
        boxes, children, order = T["boxes"], T["children"], T["order"]
        nt = dsc["triangles"].size // 3
        assert sorted(order.tolist()) == list(range(nt)), name
        assert 1 <= T["levels"] <= (cap or 24)
        if name in mf.DEEP:
            assert T["levels"] == mf.DEEP_LEVELS == 24, name
        verts = dsc["mesh_vertices"].reshape(-1, 3)[dsc["triangles"].reshape(-1, 3)]     # [nt, 3, 3]
        seen = np.zeros(nt, np.int32)
        visited = np.zeros(len(children), np.int32)
        stack = [(0, 1, None)]
        deepest = 0
        while stack:
            node, level, parent_box = stack.pop()
            visited[node] += 1
            deepest = max(deepest, level)
            for c in range(2):
                lo, hi = boxes[node, c, 0], boxes[node, c, 1]
                ch = int(children[node, c])
                if ch < 0 and (~ch & 7) == 0:
                    continue                                       # the empty child of a one-leaf tree
                if parent_box is not None:
                    assert np.all(lo >= parent_box[0]) and np.all(hi <= parent_box[1]), name
                if ch >= 0:
                    stack.append((ch, level + 1, (lo, hi)))
                else:
                    first, cnt = (~ch) >> 3, (~ch) & 7
                    assert 1 <= cnt <= 4, name
                    ids = order[first:first + cnt]
                    seen[ids] += 1
                    # strictly inside: the boxes are widened by one ulp
                    assert np.all(verts[ids] > lo) and np.all(verts[ids] < hi), name
        assert np.all(seen == 1), name
        assert np.all(visited == 1), name
        assert deepest == T["levels"], name


def test_sanitizer_standalone(pkg, scenes, tmp_path):
    """tests/cpp/mesh_bvh_check.cpp with mesh_bvh.cpp under ASan + UBSan as a
    program of its own: the fixture, the deep mesh (24 inner levels) with its
    local rays, the ladder (24 inner levels and a walk that fills the stack as
    far as such a tree can: slot 22), and 20 000 random triangles with
    repeated vertices, 10 000 rays in both modes."""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler on this machine")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # the runtimes linked into the program where the compiler can (nothing is preloaded)
    static = ["-static-libasan", "-static-libubsan"] if "g++" in Path(cxx).name else ["-static-libsan"]
    r = subprocess.run([cxx, *flags, *static, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode == 0:
        flags += static
    else:
        r = subprocess.run([cxx, *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0:
        reason = "the sanitizer runtime is absent from this machine: " + r.stderr.strip()[-300:]
        print(reason)
        pytest.skip(reason)
    o, d, _ = mf.rays(scenes)
    desc = mf.torus_desc(scenes)
    deep = mf.deep_desc(pkg, "wide")
    do, dd = mf.deep_rays("wide", "local")
    ladder = mf.ladder_desc(pkg)
    lo, ld = mf.ladder_rays()
    fx, dfx, lfx = tmp_path / "fixture.bin", tmp_path / "deep.bin", tmp_path / "ladder.bin"
    for path, dsc, ro, rd, mint in ((fx, desc, o, d, mf.MINT), (dfx, deep, do, dd, mf.MINT),
                                    (lfx, ladder, lo, ld, mf.LADDER_MINT)):
        with open(path, "wb") as f:
            np.asarray([dsc["mesh_vertices"].size // 3, dsc["triangles"].size // 3, len(ro)], np.int32).tofile(f)
            np.asarray([mint], np.float32).tofile(f)
            dsc["mesh_vertices"].tofile(f)
            dsc["triangles"].tofile(f)
            ro.tofile(f)
            rd.tofile(f)
    csrc = ROOT / "sdmm-mitsuba_amd" / "csrc"
    exe = tmp_path / "mesh_bvh_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", *flags, f"-I{csrc}",
                    str(ROOT / "tests" / "cpp" / "mesh_bvh_check.cpp"), str(csrc / "mesh_bvh.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe), str(fx), str(dfx), str(lfx)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0
    assert "mesh_bvh_check ok" in r.stdout
    assert "2048 triangles, 24 levels" in r.stdout
    # the ladder's walk writes the last slot a tree of 24 inner levels can reach (a level-24 node pushes nothing)
    assert f"{ladder['triangles'].size // 3} triangles, 24 levels" in r.stdout and "deepest stack slot 22" in r.stdout
    prim, t = _host(pkg, ladder, lo, ld, 0, mint=mf.LADDER_MINT)
    got = np.fromfile(tmp_path / "ladder.bin.out", np.int32)
    assert np.array_equal(got[:len(lo)], prim) and (prim >= 0).mean() > 0.9
    assert np.array_equal(got[len(lo):].view(np.float32).view(np.uint32), t.view(np.uint32))
    # the program's hits on the deep mesh are the library's
    prim, t = _host(pkg, deep, do, dd, 0)
    got = np.fromfile(tmp_path / "deep.bin.out", np.int32)
    assert np.array_equal(got[:len(do)], prim) and (prim >= 0).mean() > 0.9
    assert np.array_equal(got[len(do):].view(np.float32).view(np.uint32), t.view(np.uint32))
    # the program's hits on the fixture are the library's
    prim, t = _host(pkg, {k: v for k, v in desc.items() if k not in ("quads", "bsdf")}, o, d, 0)
    got = np.fromfile(tmp_path / "fixture.bin.out", np.int32)
    assert np.array_equal(got[:len(o)], prim)
    assert np.array_equal(got[len(o):].view(np.float32).view(np.uint32), t.view(np.uint32))


# ---- the deep mesh: a BVH of 24 inner levels over six decades of size ------------------
DEEP_CASES = [("wide", "local"), ("narrow", "local"), ("narrow", "outside"), ("ladder", "axial")]


def _deep_case(pkg, which, kind):
    """(description, o, d, mint) of a deep-mesh case."""
    if which == "ladder":
        return (mf.ladder_desc(pkg), *mf.ladder_rays(), mf.LADDER_MINT)
    return (mf.deep_desc(pkg, which), *mf.deep_rays(which, kind), mf.MINT)


def _half_maxt(t):
    """A finite maxt that cuts about half the hits: their median distance."""
    return float(np.median(t[np.isfinite(t)]))


@pytest.mark.parametrize("which,kind", DEEP_CASES)
def test_deep_walk_equals_loop(pkg, which, kind):
    """Mode 0 == mode 1 bitwise on (prim, t) with the stack as deep as a tree
    can make it, at maxt = inf and at a maxt that cuts about half the hits;
    mint == t and maxt == t both exclude the hit."""
    desc, o, d, mint = _deep_case(pkg, which, kind)

    def host(*a, **kw):
        return _host(*a, **{"mint": mint, **kw})
    walk, loop = host(pkg, desc, o, d, 0), host(pkg, desc, o, d, 1)
    assert _same(walk, loop)
    prim, t = walk
    assert (prim >= 0).mean() > 0.9                       # the rays are aimed
    assert np.all(np.isinf(t[prim < 0])) and np.all(t[prim >= 0] > mint)
    cut = _half_maxt(t)
    wc, lc = host(pkg, desc, o, d, 0, maxt=cut), host(pkg, desc, o, d, 1, maxt=cut)
    assert _same(wc, lc)
    assert 0.3 < (wc[0] >= 0).mean() / (prim >= 0).mean() < 0.7
    assert np.all(wc[1][wc[0] < 0] == np.float32(cut))    # (t = maxt without a hit)
    # the interval is open at both ends (the triangles are disjoint: no other t on the same one)
    hits = np.flatnonzero(prim >= 0)
    for k in hits[:: max(1, len(hits) // 12)]:
        ok, dk, tk = o[k:k + 1], d[k:k + 1], t[k]
        for mode in (0, 1):
            assert host(pkg, desc, ok, dk, mode, maxt=tk)[0][0] != prim[k]
            assert host(pkg, desc, ok, dk, mode, mint=tk)[0][0] != prim[k]
            inside = host(pkg, desc, ok, dk, mode, mint=np.nextafter(tk, np.float32(0)),
                          maxt=np.nextafter(tk, np.float32(np.inf)))
            assert inside[0][0] == prim[k] and inside[1][0] == tk


def _winners64(desc, o, d, mint=mf.MINT, chunk=256):
    """The float64 restatement's closest hit per ray, in chunks of rays (the
    deep meshes have thousands of triangles): (winner, -1 without a hit; its t;
    ambiguous by the rule of test_against_float64; the numpy float32
    restatement's t on the same primitive)."""
    win, tw, amb, t32w = [], [], [], []
    for b in range(0, len(o), chunk):
        oc, dc = o[b:b + chunk], d[b:b + chunk]
        t64, m64 = _f64_reference(desc, oc, dc, mint=mint)
        rows = np.arange(len(oc))
        two = np.argpartition(t64, 1, 1)[:, :2]
        ta, tb = t64[rows, two[:, 0]], t64[rows, two[:, 1]]
        w = np.where(ta <= tb, two[:, 0], two[:, 1])
        t1, t2 = np.minimum(ta, tb), np.maximum(ta, tb)
        hit = np.isfinite(t1)
        with np.errstate(invalid="ignore"):
            amb.append(hit & ((np.isfinite(t2) & (t2 - t1 < 1e-5 * t1)) | (m64[rows, w] < 1e-5)))
        win.append(np.where(hit, w, -1))
        tw.append(t1)
        t32w.append(_f64_reference(desc, oc, dc, np.float32, mint=mint)[0][rows, w])
    return np.concatenate(win), np.concatenate(tw), np.concatenate(amb), np.concatenate(t32w)


@pytest.mark.parametrize("which", ["wide", "narrow"])
def test_deep_against_float64(pkg, which, plog):
    """The local rays of the deep meshes against the float64 restatement, by
    the rule of test_against_float64: the same primitive on every unambiguous
    ray, at most 0.5 % ambiguous, t within 4x the numpy float32 restatement's
    own worst error on these rays (6.7e-5 relative on the wide mesh when this
    was written).  The outside rays are not compared with float64: at that
    ratio of distance to size the float32 triangle test itself is unreliable."""
    desc = mf.deep_desc(pkg, which)
    o, d = mf.deep_rays(which, "local")
    if which == "narrow":
        o, d = o[:1024], d[:1024]                         # (8192 triangles a ray in numpy)
    prim, t = _host(pkg, desc, o, d, 0)
    win, tw, ambiguous, t32w = _winners64(desc, o, d)
    share = ambiguous.mean()
    print(f"{which}: ambiguous rays: {int(ambiguous.sum())} of {len(o)} ({share:.4%})")
    plog(f"mesh_deep_{which}_ambiguous_share", share, 0.005)
    assert share <= 0.005
    clear = ~ambiguous
    wrong = int(np.sum(prim[clear] != win[clear]))
    print(f"{which}: primitive mismatches on clear rays: {wrong}")
    assert wrong == 0
    sel = clear & (win >= 0)
    assert sel.mean() > 0.9
    ok32 = sel & np.isfinite(t32w)
    err32 = float(np.max(np.abs(t32w[ok32].astype(np.float64) - tw[ok32]) / tw[ok32]))
    err = float(np.max(np.abs(t[sel].astype(np.float64) - tw[sel]) / tw[sel]))
    print(f"{which}: relative t error: library {err:.3e}, numpy float32 restatement {err32:.3e} "
          f"(bound 4x = {4 * err32:.3e})")
    plog(f"mesh_deep_{which}_t_rel_err", err, 4 * err32, float32_restatement=err32)
    assert err32 > 0
    assert err <= 4 * err32


def test_cap_independence(pkg):
    """The hits do not depend on the cap on inner levels: the deep mesh built
    with max_levels 9, 12, 16 and 24 (SAH splits refused where they would not
    leave room under the cap) answers bitwise alike; 2048 triangles need 9
    median levels, so a cap of 8 is refused."""
    desc = mf.deep_desc(pkg, "wide")
    o = np.concatenate([mf.deep_rays("wide", "local")[0], mf.deep_rays("narrow", "outside")[0]])
    d = np.concatenate([mf.deep_rays("wide", "local")[1], mf.deep_rays("narrow", "outside")[1]])
    ref = pkg.intersect_host(desc, o, d, mf.MINT, np.inf, 1)
    assert (ref[0] >= 0).mean() > 0.5
    for cap in (9, 12, 16, 24):
        assert pkg.mesh_bvh_dump(desc, max_levels=cap)["levels"] == cap      # the fallback is what holds it there
        got = pkg.intersect_host(desc, o, d, mf.MINT, np.inf, 0, max_levels=cap)
        assert _same(got, ref), cap
    assert _same(pkg.intersect_host(desc, o, d, mf.MINT, np.inf, 0), ref)
    for call in (lambda: pkg.mesh_bvh_dump(desc, max_levels=8),
                 lambda: pkg.intersect_host(desc, o[:1], d[:1], mf.MINT, np.inf, 0, max_levels=8)):
        with pytest.raises(pkg.SDMMError, match="deeper than the traversal stack"):
            call()


# ---- edge rays -------------------------------------------------------------------------
@pytest.mark.parametrize("mint", [1e-4, 1e-3])
def test_hard_rays_on_the_torus(pkg, scenes, mint):
    """Grazing rays, rays leaving the surface, -0.0 components, the zero
    direction and non-finite rays: walk == loop bitwise; the zero direction
    and the non-finite rays hit nothing, and the rays beside them answer as in
    a batch without them."""
    o, d, kinds = mf.hard_rays(scenes)
    desc = mf.torus_desc(scenes)
    for maxt in (np.inf, 2.5):
        walk, loop = _host(pkg, desc, o, d, 0, mint, maxt), _host(pkg, desc, o, d, 1, mint, maxt)
        assert _same(walk, loop), maxt
    prim, t = _host(pkg, desc, o, d, 0, mint)
    sp = kinds["special"]
    assert np.all(prim[sp] == -1) and np.all(np.isposinf(t[sp]))
    keep = np.ones(len(o), bool)
    keep[sp] = False
    alone = _host(pkg, desc, o[keep], d[keep], 0, mint)
    assert _same((prim[keep], t[keep]), alone)
    assert np.all(t[prim >= 0] > mint) and np.all(np.isposinf(t[prim < 0]))
    # the families do what they are for: grazing rays meet the torus (ids 3 +),
    # most surface rays leave it for another primitive or nothing, never for t <= mint
    assert (prim[kinds["grazing"]] >= 3).mean() > 0.5
    down = prim[kinds["negzero"]][keep[kinds["negzero"]]]              # (the floor is under all of them)
    assert (down >= 3).mean() > 0.3 and (down >= 0).all()
    surf = prim[kinds["surface"]]
    assert (surf >= 0).mean() > 0.5 and (surf >= 3).mean() > 0.2         # (upward ones leave the scene)


def test_flat_grid_vertices_edges_and_plane(pkg):
    """Rays through every vertex and every edge midpoint of a flat grid hit at
    exactly t = 1 and report the lowest id among the triangles that share the
    point; rays lying in the grid's plane hit nothing."""
    v, tr = mf.flat_grid()
    desc = mf.base_desc(v, tr, quads=False)
    o, d, expected = mf.flat_grid_rays()
    for mode in (0, 1):
        prim, t = _host(pkg, desc, o, d, mode)
        assert np.array_equal(prim, expected), mode
        assert np.all(t == np.float32(1.0)), mode
    oi, di = mf.flat_grid_inplane_rays()
    for mode in (0, 1):
        prim, t = _host(pkg, desc, oi, di, mode)
        assert np.all(prim == -1) and np.all(np.isposinf(t)), mode


def test_tie_between_quad_and_triangle(pkg):
    """A quad and a coplanar triangle at exactly the same distance: the quad,
    the lower id, wins (tri_consider's rule) in both modes."""
    desc = mf.tie_desc()
    o, d, expected = mf.tie_rays()
    # the triangle alone is hit at exactly the quad's distance
    alone = {k: v for k, v in desc.items() if k not in ("quads", "bsdf")}
    pa, ta = _host(pkg, alone, o[:4], d[:4], 0)
    assert np.all(pa == 0) and np.all(ta == np.float32(1.0))
    for mode in (0, 1):
        prim, t = _host(pkg, desc, o, d, mode)
        assert np.array_equal(prim, expected), mode
        assert np.all(t[expected >= 0] == np.float32(1.0)) and np.all(np.isposinf(t[expected < 0]))


# ---- the scale envelope ----------------------------------------------------------------
def test_scale_envelope(pkg, plog):
    """Origins 3000 units away from triangles down to 1e-3 in size: past a
    ratio of distance to size of about 1e6 Moeller-Trumbore's cancellation
    makes the loop report hits that are not there, which the walk never
    visits.  Walk != loop is allowed only on rays where the loop's winner is
    numerically unfounded -- the float64 restatement puts the ray outside that
    triangle, or the loop's t is more than 1e-4 relative from the float64 t --
    and on at most 0.1 % of the batch (2 in 100 000 when this was written)."""
    desc = mf.deep_desc(pkg, "wide")
    o, d = mf.deep_rays("wide", "outside", 20000, 4321)
    (pw, tw), (pl, tl) = _host(pkg, desc, o, d, 0), _host(pkg, desc, o, d, 1)
    differ = np.flatnonzero((pw != pl) | (tw.view(np.uint32) != tl.view(np.uint32)))
    print(f"walk != loop on {len(differ)} of {len(o)} outside rays of the 1e-3..1e3 mesh")
    plog("mesh_envelope_walk_ne_loop_share", len(differ) / len(o), 1e-3, rays=len(o), differ=len(differ))
    assert len(differ) <= 1e-3 * len(o)
    for k in differ:
        assert pl[k] >= 0, f"ray {k}: the loop reports no hit, the walk {pw[k]}"     # the walk visits a subset
        t64, _ = _f64_reference(desc, o[k:k + 1], d[k:k + 1])
        t_ref = t64[0, pl[k]]
        founded = np.isfinite(t_ref) and abs(float(tl[k]) - t_ref) <= 1e-4 * t_ref
        assert not founded, f"ray {k}: loop ({pl[k]}, {tl[k]}) is sound (float64 t {t_ref}), walk ({pw[k]}, {tw[k]})"
