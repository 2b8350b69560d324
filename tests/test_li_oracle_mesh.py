"""CPU: the oracle's triangles (oracle/sdmm_oracle_li.inc: li_tri_intersect,
the closest-hit rule of li_intersect, the mesh in li_scene) -- what the device
Li's mesh path is compared with in tests/test_gpu_li_oracle_mesh.py -- shown
right on their own:

  * or_li_intersect (a loop over every triangle, no BVH) == intersect_host bit
    for bit on (prim, t): the fixture's four meshes and 4099 rays, a mesh-only
    description, and hand-made ties;
  * the oracle's Li on a convex diffuse body in a furnace returns rho, with
    quads as emitters and with emissive triangles alone;
  * threads do not change results on the torus scene."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import mesh_fixture as mf  # noqa: E402
from test_gpu_mesh import RHO, _convex_furnace, _mean_vs_rho, _triangle_furnace  # noqa: E402

LEAF = (np.float32([[0, 0, 0, 1, 1, 1]]), np.int32([[-1, -1]]))


def _equal(pkg, oracle, desc, o, d, mint=mf.MINT, maxt=np.inf):
    hp, ht = pkg.intersect_host(desc, o, d, mint, maxt, 1)      # the library's loop over all triangles
    bp, bt = pkg.intersect_host(desc, o, d, mint, maxt, 0)      # and its BVH
    op, ot = oracle.li_intersect(desc, o, d, mint, maxt)
    assert np.array_equal(op, hp) and np.array_equal(ot.view(np.uint32), ht.view(np.uint32))
    assert np.array_equal(op, bp) and np.array_equal(ot.view(np.uint32), bt.view(np.uint32))
    return op, ot


@pytest.mark.parametrize("which", ["torus", "one", "five", "doubled", "mesh_only"])
def test_oracle_intersect_equals_host_bitwise(pkg, oracle, scenes, which):
    if which == "torus":
        desc = mf.torus_desc(scenes)
    elif which == "mesh_only":
        desc = mf.base_desc(*scenes.torus_mesh(24, 12, 1.0, 0.4), quads=False)
        assert "quads" not in desc
    else:
        desc = dict(mf.small_descs(scenes))[which]
    o, d, kinds = mf.rays(scenes)
    prim, t = _equal(pkg, oracle, desc, o, d)
    nq = 0 if which == "mesh_only" else 3
    assert (prim >= nq).any() and (prim < 0).any()
    assert prim[kinds["miss"]] == -1 and np.isinf(t[kinds["miss"]])
    if which == "doubled":
        assert prim.max() < nq + 576                            # the lower id of each pair
    if which not in ("one", "five"):
        assert (prim >= nq).sum() > 2000
    # a finite maxt: the hits beyond it are gone, t reports maxt
    prim2, t2 = _equal(pkg, oracle, desc, o, d, maxt=2.5)
    assert ((prim2 == -1) & (prim >= 0)).any() and (t2[prim2 < 0] == np.float32(2.5)).all()


def test_tie_rules(pkg, oracle):
    """Exactly equal t: a quad beats a coplanar triangle (quads come first),
    and of two identical triangles the lower id wins, in both orders of the
    triangle list; a nearer triangle still beats the quad."""
    quad = np.float32([0, 0, 0, 1, 0, 0, 0, 1, 0])                     # z = 0, normal +z
    v = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 0.5], [1, 0, 0.5], [0, 1, 0.5]])
    o = np.float32([[0.25, 0.25, 1.0], [0.25, 0.25, -1.0]])
    d = np.float32([[0, 0, -1.0], [0, 0, 1.0]])
    coplanar, near = [0, 1, 2], [3, 4, 5]
    for tris, want in (([coplanar, coplanar], [0, 0]), ([coplanar, near], [2, 0]), ([near, coplanar], [1, 0]),
                       ([near, near], [1, 0])):
        desc = {"quads": quad, "bsdf": np.zeros(1, np.int32), "reflectance": np.float32([0.5] * 3),
                "mesh_vertices": v.reshape(-1), "triangles": np.int32(tris).reshape(-1),
                "tri_bsdf": np.zeros(2, np.int32)}
        prim, t = _equal(pkg, oracle, desc, o, d)
        assert list(prim) == want, (tris, prim)
        assert t[1] == 1.0 and t[0] == (1.0 if want[0] == 0 else 0.5)
    # two identical triangles and no quad: id 0 in either order (the lists are equal: the ids swap roles)
    for tris in ([coplanar, coplanar, near], [near, coplanar, coplanar]):
        desc = {"reflectance": np.float32([0.5] * 3), "mesh_vertices": v.reshape(-1),
                "triangles": np.int32(tris).reshape(-1), "tri_bsdf": np.zeros(3, np.int32)}
        prim, t = _equal(pkg, oracle, desc, o[1:], d[1:])               # from below: the coplanar pair first
        assert prim[0] == tris.index(coplanar) and t[0] == 1.0


def _image(r):
    import torch
    return torch.from_numpy(r["image"])


def test_convex_furnace_known_answer(oracle, scenes, plog):
    """A convex diffuse body in a uniform furnace returns exactly rho
    (_mean_vs_rho's rule), one bounce a path, every vertex on a triangle;
    with the normals flipped the body is black."""
    desc = _convex_furnace(scenes)
    r = oracle.li_render(desc, *LEAF, spp=8, seed=2101, threads=4)
    _mean_vs_rho(_image(r), "oracle_bsdf", plog)
    assert (r["hit_bsdf"][0] == 1).all() and (r["hit_bsdf"][1:] == -1).all() and (r["nv"] == 1).all()
    # the scene box reaches over the quads alone here; the vertex positions lie on the unit sphere's hull
    c = r["rec"][7:10, 0] * 6.0 - 3.0
    rad = np.sqrt((c.astype(np.float64) ** 2).sum(0))
    assert rad.max() <= 1.0 + 1e-5 and rad.min() > 0.85
    flipped = oracle.li_render(_convex_furnace(scenes, flip=True), *LEAF, spp=2, seed=2102)
    assert np.abs(flipped["image"]).max() == 0.0


def test_triangle_furnace_known_answer(oracle, scenes, plog):
    """No quad at all (n_quads = 0): emissive triangles light the body to rho;
    without the body the image is the radiance; with the box's normals flipped
    it is 0."""
    desc = _triangle_furnace(scenes)
    assert "quads" not in desc
    r = oracle.li_render(desc, *LEAF, spp=8, seed=2201, threads=4)
    _mean_vs_rho(_image(r), "oracle_triangle_emitters_bsdf", plog)
    assert (r["hit_bsdf"][0] == 1).all() and RHO == 0.6
    seen = oracle.li_render(_triangle_furnace(scenes, body=False), *LEAF, spp=2, seed=2202)["image"]
    assert seen.min() == 1.0 and seen.max() == 1.0
    out = oracle.li_render(_triangle_furnace(scenes, flip_box=True), *LEAF, spp=2, seed=2203)["image"]
    assert np.abs(out).max() == 0.0


def test_description_without_mesh_fields_is_unchanged(oracle, scenes):
    """The mesh fields with no triangle in them: the render of the plain description."""
    plain = scenes.cornell_box(32, 18)
    v, _ = scenes.convex_mesh()
    with_fields = {**plain, "mesh_vertices": v.reshape(-1) * 100.0, "triangles": np.zeros(0, np.int32),
                   "tri_bsdf": np.zeros(4, np.int32)}
    a = oracle.li_render(plain, *LEAF, spp=2, seed=31)
    b = oracle.li_render(with_fields, *LEAF, spp=2, seed=31)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_threads_do_not_change_results_torus(oracle, scenes):
    desc = scenes.torus_scene(32, 18, 24, 12)
    a = oracle.li_render(desc, *LEAF, spp=2, rr_depth=3, seed=3, threads=1)
    b = oracle.li_render(desc, *LEAF, spp=2, rr_depth=3, seed=3, threads=5)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    names = ["Room", "Floor", "Torus", "Glass", "Light"]
    assert (a["hit_bsdf"] == names.index("Torus")).sum() > 20 and (a["inside"] == 1).sum() > 20
    # the vertices saved at torus bounces lie on the torus (room box: smin (-4, 0, -4), extent 8; no
    # delta lobe here, so vertex v is bounce v): within the tube's radius of its centre circle
    V = a["rec"].shape[1]
    on_torus = (a["hit_bsdf"][:V] == names.index("Torus")) & (np.arange(V)[:, None] < a["nv"][None, :])
    p = a["rec"][7:10][:, on_torus].astype(np.float64) * 8.0 + np.array([-4.0, 0.0, -4.0])[:, None]
    tube = np.hypot(np.hypot(p[0], p[2]) - 1.0, p[1] - 0.45)
    # (24 x 12 flat facets: a chord on the inner ring lies up to 0.6 (1 - cos(pi / 24)) = 0.0052 outside the tube)
    assert p.shape[1] > 20 and tube.max() <= 0.406 and tube.min() > 0.36
