"""GPU: a Scene's per-render buffers (the path, query and vertex planes of one
device block, regrown when a render needs more paths or more vertex slots, and
the extended learned-BSDF table of a product-sampling render) hold no state
between renders: a sequence of renders on one Scene that grows the path count,
then the vertex slots, then shrinks both inside the kept capacity gives, render
by render, bitwise what the same render gives on a fresh Scene.

Two scenes at 16 x 9 pixels: the Cornell box with a rough conductor (a
material with per-query lobes: product sampling extends the learned-BSDF
table) and the torus scene with the smooth materials and vertex normals (the
eta planes and the shading / geometric normal planes together).  Unguided,
and guided with product sampling by untrained (hemisphere-initialised)
mixtures on a tree split to depth 1.

The RNG is counter based, so equality is exact: the image, the image of
squares, the vertex counts and every saved vertex are compared byte for byte.
The vertex slots past a path's count are never written by a render (device
memory as allocated, on either Scene) and are left out.  (The box's lamp is
small: at these sizes its paths meet it in no render, so its images are black
and its vertices carry the comparison; the torus scene's images are lit in
every render.  The test prints the count.)
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, K = 16, 9, 16
# (spp, saved_vertices): more paths, then more vertex slots, then both back inside the kept capacity
SEQUENCE = [(1, 3), (4, 3), (4, 6), (1, 3)]


def _desc(scenes, name):
    if name == "cornell_conductor":
        return scenes.cornell_box(W, H, conductor=("TallBox",))
    desc = scenes.torus_scene(W, H, nu=8, nv=4, smooth=True, smooth_normals=True)
    assert desc["mesh_normals"].size == desc["mesh_vertices"].size
    return desc


def _guide(pkg, synth, scene):
    """(tree split to depth 1, one hemisphere-initialised mixture per leaf)."""
    _, _, tmin, tmax = scene.normalization()
    tree = pkg.STree(tmin, tmax)
    tree.split_to_depth(1)
    aabb, child, _ = tree.nodes()
    rng = np.random.default_rng(16)
    mixes = [None] * tree.num_nodes
    for v in range(tree.num_nodes):
        if child[v, 0] >= 0:
            continue
        pos = rng.uniform(aabb[v, :3], aabb[v, 3:], (K // 8, 3)).astype(np.float32)
        nrm = rng.normal(size=(K // 8, 3))
        nrm = (nrm / np.linalg.norm(nrm, axis=1)[:, None]).astype(np.float32)
        m = pkg.SDMM(K)
        m.init_hemisphere(pos, nrm, synth.DEPTH_PRIOR, synth.SPATIAL_DISTANCE, 11 + v)
        mixes[v] = m
    assert sum(m is not None for m in mixes) == tree.leaf_nodes == 8
    return tree, mixes


def _render(scene, tree, mixes, table, spp, saved, step, gpu):
    """One render as bytes: image, image of squares, vertex counts, saved vertices."""
    import torch
    img = torch.zeros(3, H, W, device=gpu)
    sqr = torch.zeros(3, H, W, device=gpu)
    kw = dict(node_mix=mixes, guided=True, learned_bsdf=table) if mixes is not None else {}
    _, verts, st = scene.render(tree, spp=spp, max_depth=saved + 1, saved_vertices=saved, seed=40 + step,
                                image=img, image_sqr=sqr, **kw)
    rec, nv = verts.to_numpy()
    P = W * H * spp
    assert st["paths"] == P == nv.size and verts.s.max_vertices == saved
    rec = rec.reshape(16, saved, P)
    used = np.arange(saved)[:, None] < nv[None, :]
    assert 0 < nv.max() <= saved
    return (img.cpu().numpy().tobytes(), sqr.cpu().numpy().tobytes(), nv.tobytes(), rec[:, used].tobytes(),
            st["segments"], st["guided_queries"])


@pytest.mark.parametrize("guided", [False, True], ids=["unguided", "product"])
@pytest.mark.parametrize("name", ["cornell_conductor", "torus_smooth_normals"])
def test_regrown_buffers_equal_a_fresh_scene(pkg, scenes, synth, gpu, name, guided):
    desc = _desc(scenes, name)
    scene = pkg.Scene(desc)
    tree, mixes = _guide(pkg, synth, scene)
    table = None
    if guided:
        learned = scenes.diffuse_learned_bsdf(len(desc["reflectance"]) // 3)
        table = pkg.BsdfTable(*learned[:3], device=gpu, diffuse=learned[3])
    else:
        mixes = None
    queries = lit = 0
    for step, (spp, saved) in enumerate(SEQUENCE):
        got = _render(scene, tree, mixes, table, spp, saved, step, gpu)
        fresh = pkg.Scene(desc)
        want = _render(fresh, tree, mixes, table, spp, saved, step, gpu)
        for what, a, b in zip(("image", "image_sqr", "nv", "saved vertices", "segments", "guided queries"), got, want):
            assert a == b, (name, guided, step, what)
        # (at 16 x 9 and 1 spp the box's small lamp may light no path: the vertices carry the comparison there)
        assert any(got[3]) and got[4] > 0
        lit += any(got[0])
        queries += got[5]
    print(f"{name}, {'product' if guided else 'unguided'}: {lit} of {len(SEQUENCE)} images lit, {queries} guided queries")
    assert (queries > 0) == guided
