"""Host: vertex normals on meshes (sdmm_scene_desc.mesh_normals) --
sdmm_scene_shading_host against the numpy float32 restatement of the hit-normal
rule (tests/shading_cases.py), the validation messages, scenes.vertex_normals
(Mitsuba's angle-weighted computeNormals) and mirror_z with normals.  No GPU."""
import numpy as np
import pytest

import mesh_fixture as mf
import shading_cases as sc


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def all_cases(scenes):
    return sc.cases(scenes)


@pytest.mark.parametrize("name", ["torus_benign", "torus_hard", "disagree", "flip", "unnormalised", "vanish"])
def test_shading_host_equals_restatement(pkg, all_cases, name):
    desc, o, d = all_cases[name]
    prim, t, ns, ng = pkg.shading_host(desc, o, d, mint=mf.MINT)
    p0, t0 = pkg.intersect_host(desc, o, d, mint=mf.MINT)
    assert np.array_equal(prim, p0) and np.array_equal(_bits(t), _bits(t0))
    want_ns, want_ng = sc.restate(desc, o, d, prim)
    bad = np.nonzero((_bits(ns) != _bits(want_ns)).any(1) | (_bits(ng) != _bits(want_ng)).any(1))[0]
    assert not len(bad), (name, bad[:5], ns[bad[:2]], want_ns[bad[:2]], ng[bad[:2]], want_ng[bad[:2]])
    # misses carry zeros, hits unit vectors
    miss = prim < 0
    assert (ns[miss] == 0).all() and (ng[miss] == 0).all()
    assert np.abs(np.linalg.norm(ns[~miss].astype(np.float64), axis=1) - 1).max(initial=0) < 1e-6
    assert np.abs(np.linalg.norm(ng[~miss].astype(np.float64), axis=1) - 1).max(initial=0) < 1e-6
    assert (np.einsum("ij,ij->i", ns[~miss], ng[~miss]) >= 0).all()       # ng follows ns
    # the BVH and the loop over all triangles agree
    prim1, t1, ns1, ng1 = pkg.shading_host(desc, o, d, mint=mf.MINT, mode=1)
    assert np.array_equal(prim, prim1) and np.array_equal(_bits(t), _bits(t1))
    assert np.array_equal(_bits(ns), _bits(ns1)) and np.array_equal(_bits(ng), _bits(ng1))


def test_cases_reach_what_they_are_for(pkg, scenes, all_cases):
    n_quads = 3
    desc, o, d = all_cases["torus_benign"]
    prim, _, ns, ng = pkg.shading_host(desc, o, d, mint=mf.MINT)
    tri = prim >= n_quads
    assert tri.sum() > 1500 and ((prim >= 0) & ~tri).sum() > 50 and (prim < 0).sum() > 50
    # smooth normals are not the face normals: they differ from ng on most triangle hits
    assert (np.abs(ns[tri] - ng[tri]).max(1) > 1e-3).mean() > 0.9
    # quads: the face normal twice
    quad = (prim >= 0) & ~tri
    assert np.array_equal(_bits(ns[quad]), _bits(ng[quad]))
    # without normals every hit has ns = ng = today's face normal, which is ng of the smooth case
    bare = {k: v for k, v in desc.items() if k != "mesh_normals"}
    _, _, fs, fg = pkg.shading_host(bare, o, d, mint=mf.MINT)
    assert np.array_equal(_bits(fs), _bits(fg)) and np.array_equal(_bits(fg), _bits(ng))
    # normals against the winding: ng is the negated face normal, ns the negated ns
    _, _, ns_d, ng_d = pkg.shading_host(all_cases["disagree"][0], o, d, mint=mf.MINT)
    assert np.array_equal(_bits(ng_d[tri]), _bits(-ng[tri])) and np.array_equal(_bits(ns_d[tri]), _bits(-ns[tri]))
    # tri_flip_normals negates ns (and ng with it); the winding is left alone
    fdesc = all_cases["flip"][0]
    _, _, ns_f, ng_f = pkg.shading_host(fdesc, o, d, mint=mf.MINT)
    flipped = np.zeros(len(prim), bool)
    flipped[tri] = fdesc["tri_flip_normals"][prim[tri] - n_quads] != 0
    assert flipped.sum() > 500
    assert np.array_equal(_bits(ns_f[flipped]), _bits(-ns[flipped])) and np.array_equal(_bits(ng_f[flipped]), _bits(-ng[flipped]))
    assert np.array_equal(_bits(ns_f[~flipped]), _bits(ns[~flipped]))
    # normals of other lengths: the interpolation weights change, ng does not
    _, _, ns_u, ng_u = pkg.shading_host(all_cases["unnormalised"][0], o, d, mint=mf.MINT)
    assert np.array_equal(_bits(ng_u), _bits(ng)) and not np.array_equal(_bits(ns_u[tri]), _bits(ns[tri]))


def test_vanishing_sum_falls_back_to_the_face_normal(pkg):
    desc = sc.vanish_desc()
    o, d, vanishing = sc.vanish_rays()
    prim, t, ns, ng = pkg.shading_host(desc, o, d, mint=mf.MINT)
    assert list(prim) == [0, 0, 1, 1, 0, 0, 1, 1, -1] and (t[:8] == 1.0).all()
    # the winding's face normal is (0, -1, 0); triangle 1 is flipped
    assert (ns[:2] == [0, -1, 0]).all() and (ng[:2] == [0, -1, 0]).all()
    assert (ns[2:4] == [0, 1, 0]).all() and (ng[2:4] == [0, 1, 0]).all()
    # beside the line u = 1/2 the sum is (0, +-k, 0): u < 1/2 gives +y, u > 1/2 gives -y
    assert (ns[4:6] == [0, 1, 0]).all() and (ng[4:6] == [0, 1, 0]).all()         # ng turned onto ns
    assert (ns[6] == [0, -1, 0]).all() and (ns[7] == [0, 1, 0]).all()           # flipped: ns negated
    assert np.array_equal(ns[6:8], ng[6:8])
    assert vanishing.sum() == 4


def test_validation_messages(pkg, scenes):
    desc = sc.torus_desc(scenes)
    o, d, _ = mf.rays(scenes)
    n = desc["mesh_normals"].reshape(-1, 3)

    def message(changed):
        with pytest.raises(pkg.SDMMError) as e:
            pkg.shading_host(changed, o[:4], d[:4])
        return str(e.value)
    bad = n.copy()
    bad[5, 1] = np.nan
    assert "non-finite vertex normal" in message(dict(desc, mesh_normals=bad.reshape(-1)))
    bad = n.copy()
    bad[7, 0] = np.inf
    assert "non-finite vertex normal" in message(dict(desc, mesh_normals=bad.reshape(-1)))
    bad = n.copy()
    bad[9] = 0.0
    assert "vertex normal of length 0" in message(dict(desc, mesh_normals=bad.reshape(-1)))
    with pytest.raises(pkg.SDMMError, match="3 floats per mesh vertex"):
        pkg.shading_host(dict(desc, mesh_normals=n[:-1].reshape(-1)), o[:4], d[:4])
    # mesh_normals without triangles: through the C entry (the wrapper would count the vertices)
    import ctypes as C
    sd, keep = pkg._SceneDesc(), {}
    quads_only = {k: v for k, v in desc.items() if k in ("reflectance", "quads", "bsdf")}
    pkg._fill_geometry(sd, quads_only, keep)
    one = np.asarray([0, 1, 0], np.float32)
    sd.mesh_normals = one.ctypes.data
    out = [np.zeros(3, np.float32) for _ in range(2)]
    prim, t = np.zeros(1, np.int32), np.zeros(1, np.float32)
    rc = pkg.lib().sdmm_scene_shading_host(C.byref(sd), 1, o[:1].ctypes.data, d[:1].ctypes.data, 1e-4, float("inf"), 0,
                                           prim.ctypes.data, t.ctypes.data, out[0].ctypes.data, out[1].ctypes.data)
    assert rc != 0
    with pytest.raises(pkg.SDMMError, match="mesh_normals without triangles"):
        pkg._check(rc)


def test_vertex_normals_cube(scenes):
    """An 8-vertex cube of 12 triangles: the angle weights of a face sum to
    pi / 2 at a corner whichever way its diagonal runs, so every corner's
    normal is (+-1, +-1, +-1) / sqrt(3); unweighted or area-weighted averaging
    favours the faces whose diagonal ends at the corner."""
    v = np.asarray([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float32)

    def idx(x, y, z):
        return (x > 0) * 4 + (y > 0) * 2 + (z > 0)
    tris = []
    for ax in range(3):
        for s in (-1, 1):
            a, b = [(1, 2), (2, 0), (0, 1)][ax]
            def corner(ca, cb):
                c = [0, 0, 0]
                c[ax], c[a], c[b] = s, ca, cb
                return idx(*c)
            q = [corner(-1, -1), corner(1, -1), corner(1, 1), corner(-1, 1)]
            if s < 0:
                q = q[::-1]
            # the diagonals run differently on the two faces of an axis
            tris += [(q[0], q[1], q[2]), (q[0], q[2], q[3])] if s > 0 else [(q[1], q[2], q[3]), (q[1], q[3], q[0])]
    tris = np.asarray(tris, np.int32)
    assert tris.shape == (12, 3)
    fn = np.cross(v[tris[:, 1]] - v[tris[:, 0]], v[tris[:, 2]] - v[tris[:, 0]])
    assert (np.einsum("ij,ij->i", fn, v[tris].mean(1)) > 0).all()           # outward winding
    n = scenes.vertex_normals(v, tris)
    assert n.dtype == np.float32 and np.abs(n - v / np.sqrt(3.0)).max() <= 1e-6
    # the unweighted average of the adjacent triangles' normals is not that
    un = np.zeros((8, 3))
    for t_, f in zip(tris, fn / np.linalg.norm(fn, axis=1, keepdims=True)):
        un[t_] += f
    un /= np.linalg.norm(un, axis=1, keepdims=True)
    assert np.abs(un - v / np.sqrt(3.0)).max() > 1e-2


def test_vertex_normals_torus(scenes):
    v, t, analytic = scenes.torus_mesh(24, 12, 1.0, 0.4, normals=True)
    n = scenes.vertex_normals(v, t)
    assert np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1.0).max() <= 1e-6
    assert np.abs(np.linalg.norm(analytic.astype(np.float64), axis=1) - 1.0).max() <= 1e-6
    # both are the outward normal of the same surface: within the tessellation's angle
    assert np.einsum("ij,ij->i", n, analytic).min() > np.cos(0.1)
    # to_world: the inverse transpose (a non-uniform scale and a shear)
    M = np.asarray([[2.0, 0.3, 0, 1], [0, 0.5, 0, 2], [0, 0, 1.5, 3]])
    vw, tw, nw = scenes.torus_mesh(96, 48, 1.0, 0.4, to_world=M, normals=True)
    assert np.abs(np.linalg.norm(nw.astype(np.float64), axis=1) - 1.0).max() <= 1e-6
    # (a fine mesh: the transformed mesh's own angle-weighted normals are then the surface's)
    assert np.einsum("ij,ij->i", scenes.vertex_normals(vw, tw), nw).min() > np.cos(0.05)


def test_mirror_z_twice_is_the_description(scenes):
    desc = scenes.torus_scene(64, 36, nu=24, nv=12, glass=False, smooth_normals=True)
    assert "mesh_normals" in desc
    nt = len(desc["triangles"]) // 3
    nq = len(desc["quads"]) // 9
    once = scenes.mirror_z(desc, keep=(nq + 3,))
    n0, n1 = desc["mesh_normals"].reshape(-1, 3), once["mesh_normals"].reshape(-1, 3)
    assert np.array_equal(n1[:, :2], n0[:, :2]) and np.array_equal(n1[:, 2], -n0[:, 2])
    # the triangles' flags stay (the flag negates ns itself); the kept one is toggled; quads toggle as ever
    assert once["tri_flip_normals"].sum() == 1 and once["tri_flip_normals"][3] == 1
    assert once["flip_normals"].all()
    twice = scenes.mirror_z(once, keep=(nq + 3,))
    assert set(twice) == set(desc) | {"flip_normals", "tri_flip_normals"}
    assert not twice["flip_normals"].any() and not twice["tri_flip_normals"].any() and len(twice["tri_flip_normals"]) == nt
    for k, v in desc.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(twice[k], v), k
        else:
            assert twice[k] is v or twice[k] == v, k
