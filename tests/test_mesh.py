"""Triangle meshes on the host (no GPU): sdmm_scene_intersect_host's BVH against
its brute-force loop and against a float64 restatement, the description's
validation, the BVH's shape (sdmm_mesh_bvh_dump) and a sanitizer run of the
build and the traversal as a stand-alone program."""
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


def _f64_reference(desc, o, d, dtype=np.float64):
    """Moeller-Trumbore (core/triangle.h:109-145) and the quads' plane test
    restated in numpy at `dtype`: per ray (t [nq, n_prims], inside margin [nq,
    n_prims]) -- t = inf where the primitive is missed; margin: the least
    distance of the barycentrics (quad: of its two coordinates) to an edge."""
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
        ok = (det != 0) & (u >= 0) & (u <= 1) & (vv >= 0) & (u + vv <= 1) & (t > mf.MINT)
        margin = np.minimum(np.minimum(u, vv), 1 - u - vv)
        tt = np.where(ok, t, np.inf)
        q = desc["quads"].reshape(-1, 3, 3).astype(dtype)
        n = np.cross(q[:, 1], q[:, 2])
        den = d @ n.T
        tq = ((q[None, :, 0] - o[:, None]) * n[None]).sum(-1) / den
        r = o[:, None] + tq[..., None] * d[:, None] - q[None, :, 0]
        g1 = np.cross(q[:, 2], n) / (q[:, 1] * np.cross(q[:, 2], n)).sum(-1, keepdims=True)
        g2 = np.cross(n, q[:, 1]) / (q[:, 2] * np.cross(n, q[:, 1])).sum(-1, keepdims=True)
        a, b = (r * g1[None]).sum(-1), (r * g2[None]).sum(-1)
        okq = (den != 0) & (tq > mf.MINT) & (a >= 0) & (a <= 1) & (b >= 0) & (b <= 1)
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
    box inside its parent's, the depth within the cap."""
    desc = mf.torus_desc(scenes)
    for name, dsc in [("torus", desc)] + (mf.small_descs(scenes) if cap == 0 else []):
        T = pkg.mesh_bvh_dump(dsc, max_levels=cap)
        boxes, children, order = T["boxes"], T["children"], T["order"]
        nt = dsc["triangles"].size // 3
        assert sorted(order.tolist()) == list(range(nt)), name
        assert 1 <= T["levels"] <= (cap or 24)
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
    program of its own: the fixture and 20 000 random triangles with repeated
    vertices, 10 000 rays in both modes."""
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
    fx = tmp_path / "fixture.bin"
    with open(fx, "wb") as f:
        np.asarray([desc["mesh_vertices"].size // 3, desc["triangles"].size // 3, len(o)], np.int32).tofile(f)
        desc["mesh_vertices"].tofile(f)
        desc["triangles"].tofile(f)
        o.tofile(f)
        d.tofile(f)
    csrc = ROOT / "sdmm-mitsuba_amd" / "csrc"
    exe = tmp_path / "mesh_bvh_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", *flags, f"-I{csrc}",
                    str(ROOT / "tests" / "cpp" / "mesh_bvh_check.cpp"), str(csrc / "mesh_bvh.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe), str(fx)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0
    assert "mesh_bvh_check ok" in r.stdout
    # the program's hits on the fixture are the library's
    prim, t = _host(pkg, {k: v for k, v in desc.items() if k not in ("quads", "bsdf")}, o, d, 0)
    got = np.fromfile(tmp_path / "fixture.bin.out", np.int32)
    assert np.array_equal(got[:len(o)], prim)
    assert np.array_equal(got[len(o):].view(np.float32).view(np.uint32), t.view(np.uint32))
