"""GPU: the triangle-mesh path of the device Li (the MESH variants of the
camera, loop-head, compact and shade kernels of csrc/render.hip: prim_n /
prim_bsdf / prim_emitter indexed by q - n_quads, the BVH walk, the quad-before-
triangle tie rule, the scene box over the mesh vertices, emitters on
triangles) against the CPU restatement (oracle/sdmm_oracle_li.inc: a loop over
every triangle, pinned on its own in tests/test_li_oracle_mesh.py), path by
path, in the forms of tests/test_gpu_li_oracle.py: unguided bit-exact -- also
with Russian roulette on (rr_depth = 2) -- guided and product through
_compare_guided, unchanged.

The mesh path has no device transcendental the other bitwise tests do not
rely on: zero mismatching paths.  Kind 4 appears twice: on triangles (the
Cornell box's tall box as a closed glass body of 12 triangles) and on the
quads of the torus scene's case, whose torus is diffuse; see
tests/test_gpu_li_oracle_dielectric.py on bitwise there."""
import numpy as np
import pytest

from test_bsdf_roughdielectric import ETA
from test_gpu_li_oracle import SEED, SPP, _compare_guided
from test_gpu_li_oracle_dielectric import (_assert_bitwise, _glass_counts, _guided, _roulette_deaths,
                                           _second_lobe_outside, _unguided)
from test_gpu_mesh import _triangle_furnace

pytestmark = pytest.mark.gpu


def _prims(oracle, desc, r):
    """The primitive under every saved vertex of the oracle's paths: the
    oracle's own closest hit along the segment that reached it (from the camera
    for the first).  [V, P], -1 where no vertex was saved or none was found."""
    V, P = r["rec"].shape[1:]
    q = np.asarray(desc.get("quads", np.zeros(0)), np.float64).reshape(-1, 3, 3)
    pts = [q[:, 0], q[:, 0] + q[:, 1], q[:, 0] + q[:, 2], q[:, 0] + q[:, 1] + q[:, 2]] if len(q) else []
    if np.asarray(desc.get("triangles", [])).size:
        pts.append(np.asarray(desc["mesh_vertices"], np.float64).reshape(-1, 3))
    pts = np.concatenate(pts).astype(np.float32)
    smin, snorm = pts.min(0), (pts.max(0) - pts.min(0)).max()
    pos = np.moveaxis(r["rec"][7:10], 0, -1).astype(np.float64) * snorm + smin            # [V, P, 3]
    cam = np.asarray(desc["camera_to_world"], np.float64).reshape(4, 4)[:3, 3]
    prev = np.concatenate([np.broadcast_to(cam, pos[:1].shape), pos[:-1]])
    sel = np.arange(V)[:, None] < r["nv"][None, :]
    prim, _ = oracle.li_intersect(desc, prev[sel], pos[sel] - prev[sel], 1e-3, 1.001)
    out = np.full((V, P), -1, np.int32)
    out[sel] = prim
    return out


CUBES = ("ShortBox", "TallBox")


@pytest.mark.parametrize("rr_depth", [10, 2])
def test_cornell_cubes_as_triangles_unguided_bitwise(pkg, oracle, scenes, gpu, plog, rr_depth):
    """The Cornell box with both cubes as triangles (24, behind 6 quads): the
    device Li equals the CPU Li bit for bit, with and without roulette."""
    desc = scenes.cornell_box(128, 72, mesh=CUBES)
    nq = desc["quads"].size // 9
    assert desc["triangles"].size // 3 == 24 and nq == 6
    img, rec, nv, r, (aabb, child) = _unguided(pkg, oracle, desc, rr_depth=rr_depth)
    prims = _prims(oracle, desc, r)
    ids = [list(scenes._BSDFS).index(n) for n in CUBES]
    V = rec.shape[1]
    on_tri = prims >= nq
    cube_hits = np.isin(r["hit_bsdf"][:V], ids) & (np.arange(V)[:, None] < r["nv"][None, :])
    counts = {"vertices_on_triangles": int(on_tri.sum()), "cube_bsdf_vertices": int(cube_hits.sum()),
              "saved_vertices": int(r["nv"].sum())}
    # the cubes exist as triangles only: a vertex is on a triangle where the oracle scattered at a cube BSDF
    # (but for a vertex on an edge, where the re-traced segment may find the neighbour)
    assert counts["vertices_on_triangles"] >= counts["saved_vertices"] // 20, counts
    assert (on_tri != cube_hits).sum() <= counts["saved_vertices"] // 1000, (counts, int((on_tri != cube_hits).sum()))
    if rr_depth == 2:
        r10 = oracle.li_render(desc, aabb, child, spp=SPP, seed=SEED, threads=16)
        counts["roulette_deaths"] = _roulette_deaths(r, r10)
        assert counts["roulette_deaths"] >= nv.shape[0] // 20, counts
    _assert_bitwise(plog, f"li_mesh_cornell_rr{rr_depth}_unguided", img, rec, nv, r, **counts)


def test_triangle_furnace_unguided_bitwise(pkg, oracle, scenes, gpu, plog):
    """No quad at all, emissive triangles (tri_emitter, the quads' emitter
    array absent) round a convex diffuse body: camera rays and bounce rays end
    on emitters that are triangles."""
    desc = _triangle_furnace(scenes)
    img, rec, nv, r, _ = _unguided(pkg, oracle, desc)
    assert (r["hit_bsdf"][0] == 1).all() and (r["nv"] == 1).all()
    # every path's one vertex carries the emitter's radiance over its pdf: the bounce ray met an emissive triangle
    lit = int((r["rec"][0, 0] > 0).sum())
    assert lit == nv.shape[0]
    prims = _prims(oracle, desc, r)
    assert (prims[0] >= 12).all()                           # on the body's triangles, behind the box's twelve
    _assert_bitwise(plog, "li_mesh_triangle_furnace_unguided", img, rec, nv, r, emitter_hits_on_triangles=lit)
    assert float(img.mean()) > 0.5


# ---- a kind-4 body of triangles ----------------------------------------------------
def _glass_mesh_box(scenes, alpha, w=128, h=72):
    """The Cornell box whose tall box is a closed body of 12 triangles with a
    rough-dielectric BSDF (lifted 0.02 off the floor, as the quad glass box of
    tests/test_gpu_li_oracle_dielectric.py)."""
    desc = scenes.cornell_box(w, h, mesh=("TallBox",), dielectric=("TallBox",), dielectric_lift=0.02,
                              dielectric_ior=(ETA, 1.0), dielectric_alpha=alpha)
    tb = list(scenes._BSDFS).index("TallBox")
    assert desc["triangles"].size // 3 == 12 and (desc["tri_bsdf"] == tb).all() and not (desc["bsdf"] == tb).any()
    assert desc["bsdf_params"].reshape(-1, 8)[tb, 0] == 4.0
    return desc, tb


def _glass_mesh_counts(oracle, desc, r, tb):
    """_glass_counts, and the kind-4 hits from inside at vertices whose
    primitive (the oracle's own closest hit along the segment that reached
    the vertex) is a triangle."""
    V = r["rec"].shape[1]
    nq = desc["quads"].size // 9
    live = np.arange(V)[:, None] < r["nv"][None, :]
    on_tri = _prims(oracle, desc, r) >= nq
    glass = (r["hit_bsdf"][:V] == tb) & live
    c = _glass_counts(r, [tb])
    c["glass_vertices_on_triangles"] = int((glass & on_tri).sum())
    c["inside_hits_on_triangles"] = int((glass & on_tri & (r["inside"][:V] == 1)).sum())
    # the body exists as triangles only (but for a vertex on an edge, where the re-traced segment may miss)
    assert (glass != on_tri).sum() <= c["saved_vertices"] // 1000, (c, int((glass != on_tri).sum()))
    assert c["inside_hits_on_triangles"] >= c["saved_vertices"] // 100, c
    assert c["reflected"] > 0 and c["transmitted"] > 0, c
    return c


@pytest.mark.parametrize("rr_depth", [10, 2])
def test_glass_mesh_box_unguided_bitwise(pkg, oracle, scenes, gpu, plog, rr_depth):
    """A kind-4 BSDF on triangles: two-sided hits through prim_n / prim_bsdf at
    q - n_quads, the sample in Frame(n) of a triangle's face normal from
    either side, -n saved inside the body, the crossed index through a closed
    triangle body and (rr_depth 2) the path's relative index in roulette --
    bit for bit the CPU Li's."""
    desc, tb = _glass_mesh_box(scenes, 0.1)
    img, rec, nv, r, (aabb, child) = _unguided(pkg, oracle, desc, rr_depth=rr_depth)
    c = _glass_mesh_counts(oracle, desc, r, tb)
    if rr_depth == 2:
        r10 = oracle.li_render(desc, aabb, child, spp=SPP, seed=SEED, threads=16)
        r1 = oracle.li_render(desc, aabb, child, spp=SPP, seed=SEED, rr_depth=2, threads=16, rr_eta_one=True)
        c["roulette_deaths"] = _roulette_deaths(r, r10)
        c["paths_changed_by_eta"] = int((r1["nv"] != r["nv"]).sum())
        assert c["roulette_deaths"] >= nv.shape[0] // 20 and c["paths_changed_by_eta"] >= 1, c
    _assert_bitwise(plog, f"li_mesh_glass_box_rr{rr_depth}_unguided", img, rec, nv, r, **c)


@pytest.mark.parametrize("product", [False, True], ids=["guided", "product"])
def test_glass_mesh_box_guided_li_matches_oracle(pkg, oracle, scenes, gpu, plog, product):
    """Guided and product bounces at the triangle glass body, K = 16, alpha 0.3
    (see test_glass_box_guided_li_matches_oracle on the alpha): the whole-sphere
    eval at a triangle hit, and in the product the SDMM5 conditioned at hits
    from outside, the plain conditional from inside."""
    desc, tb = _glass_mesh_box(scenes, 0.3)
    img, rec, nv, r = _guided(pkg, oracle, scenes, gpu, desc, 16, product=product)
    c = _glass_mesh_counts(oracle, desc, r, tb)
    V = rec.shape[1]
    g = (r["comps"][:V] >= 0) & (r["hit_bsdf"][:V] == tb)
    c["guide_outside"] = int((g & (r["inside"][:V] == 0)).sum())
    c["guide_inside"] = int((g & (r["inside"][:V] == 1)).sum())
    assert c["guide_outside"] > 0 and c["guide_inside"] > 0, c
    if product:
        c["second_lobe_samples"] = _second_lobe_outside(r, [tb])
        assert c["second_lobe_samples"] > 0, c
    tag = f"li_mesh_glass_box_{'product' if product else 'guided'}"
    print(f"{tag}:", c)
    plog(f"{tag}_inside_hits_on_triangles", c["inside_hits_on_triangles"], c["saved_vertices"] // 100, lower=True, **c)
    _compare_guided(oracle, plog, tag, img, rec, nv, r)


# ---- the torus scene -----------------------------------------------------------------
def _torus(scenes, alpha=None):
    """torus_scene(128, 72, 24, 12); alpha: another Beckmann alpha for the glass case."""
    desc = scenes.torus_scene(128, 72, 24, 12)
    names = ["Room", "Floor", "Torus", "Glass", "Light"]
    g = names.index("Glass")
    bp = desc["bsdf_params"].reshape(-1, 8).copy()
    assert bp[g, 0] == 4.0 and abs(bp[g, 6] - 0.05) < 1e-6
    if alpha is not None:
        bp[g, 6] = alpha
        desc["bsdf_params"] = bp.reshape(-1)
    return desc, names.index("Torus"), g


def _torus_counts(oracle, desc, r, torus, glass):
    V = r["rec"].shape[1]
    live = np.arange(V)[:, None] < r["nv"][None, :]
    nq = desc["quads"].size // 9
    prims = _prims(oracle, desc, r)
    on_torus = (r["hit_bsdf"][:V] == torus) & live
    c = {"saved_vertices": int(live.sum()), "vertices_on_torus": int(on_torus.sum()),
         "vertices_on_triangles": int((prims >= nq).sum()),
         "inside_glass_hits": int(((r["inside"][:V] == 1) & (r["hit_bsdf"][:V] == glass) & live).sum())}
    # the torus is the only mesh: the two counts name the same vertices (but for re-traced edge hits)
    assert abs(c["vertices_on_torus"] - c["vertices_on_triangles"]) <= c["saved_vertices"] // 1000, c
    assert c["vertices_on_torus"] >= c["saved_vertices"] // 100 and c["inside_glass_hits"] > 0, c
    return c


def test_torus_scene_unguided_bitwise(pkg, oracle, scenes, gpu, plog):
    """The torus scene with its own alpha (0.05).  The torus itself is diffuse:
    the scene's only kind-4 surfaces are the quads of the glass case over it
    (a kind-4 body of triangles is test_glass_mesh_box_*), so the guard counts
    vertices on the torus and hits of the case from inside.  The paths that
    reach the torus crossed the glass twice."""
    desc, torus, glass = _torus(scenes)
    img, rec, nv, r, _ = _unguided(pkg, oracle, desc)
    c = _torus_counts(oracle, desc, r, torus, glass)
    _assert_bitwise(plog, "li_mesh_torus_unguided", img, rec, nv, r, **c)


@pytest.mark.parametrize("product", [False, True], ids=["guided", "product"])
def test_torus_scene_guided_li_matches_oracle(pkg, oracle, scenes, gpu, plog, product):
    """Guided and product bounces over the torus scene (a diffuse torus under
    a kind-4 case of quads), K = 16.  The scene's
    alpha is 0.05; these two cases run at 0.3, because a guide direction that
    differs by 1e-5 between device and oracle moves the Beckmann density by
    about 6e-5 / alpha relative at theta_m = 3 alpha -- 1.2e-3 at 0.05, beyond
    _compare_guided's 1e-3, and 2e-4 at 0.3."""
    desc, torus, glass = _torus(scenes, alpha=0.3)
    img, rec, nv, r = _guided(pkg, oracle, scenes, gpu, desc, 16, product=product)
    c = _torus_counts(oracle, desc, r, torus, glass)
    V = rec.shape[1]
    c["guide_samples_on_torus"] = int(((r["comps"][:V] >= 0) & (r["hit_bsdf"][:V] == torus)).sum())
    print(f"torus {'product' if product else 'guided'}:", c)
    assert c["guide_samples_on_torus"] > 0, c
    tag = f"li_mesh_torus_{'product' if product else 'guided'}"
    plog(f"{tag}_vertices_on_torus", c["vertices_on_torus"], c["saved_vertices"] // 100, lower=True, **c)
    _compare_guided(oracle, plog, tag, img, rec, nv, r)
