"""Environment emitters in the device Li: Scene.env_eval against env_eval_host
bitwise, a constant environment against a closed cube of emitter quads (the
same paths, bitwise), known answers, the camera kernel's wiring with a varying
rotated map, guided renders of the open torus scene, and a description with
env_kind = 0 rendering as before."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import env_fixture as ef  # noqa: E402
from test_gpu_li import _check_producer, _train, _tree  # noqa: E402
from test_gpu_mesh import _lum, _sigma  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]

RHO = 0.6
RAD = np.asarray([1.0, 0.8, 0.6], np.float32)
# the film's float32 sum of up to 256 equal terms: the furnace test's slack (tests/test_gpu_mesh.py)
SLACK = 256 * 2.0 ** -24


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _planes(a, gpu):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a[:, i])).to(gpu) for i in range(3)]


_CAM = {"camera_to_world": np.asarray([-1, 0, 0, 0, 0, 1, 0, 0, 0, 0, -1, 2.5, 0, 0, 0, 1], np.float32),
        "fov_x_deg": 60.0, "near_clip": 1e-2, "width": 64, "height": 36}


def _body(scenes):
    """convex_mesh() (diffuse, rho 0.6; BSDF 1 of a table whose BSDF 0 is the
    black one of the emitter quads) seen from (0, 0, 2.5) with a 60 degree
    field of view: the body fills the middle of the image, the rays of the
    outer pixels miss it."""
    v, t = scenes.convex_mesh()
    return {**_CAM, "reflectance": np.asarray([0, 0, 0, RHO, RHO, RHO], np.float32), "mesh_vertices": v.reshape(-1),
            "triangles": t.reshape(-1), "tri_bsdf": np.ones(len(t), np.int32)}


def _body_in_emitter_cube(scenes):
    """Scene A: the body inside the closed cube [-3, 3]^3 of six inward-facing
    one-sided emitter quads, radiance RAD, reflectance 0; the camera inside."""
    cube = np.array([[3.0, 0, 0, 0], [0, 3.0, 0, 0], [0, 0, 3.0, 0]])
    quads = [np.concatenate(f) for f in scenes._cube_faces(cube)]
    return {**_body(scenes), "quads": np.asarray(quads, np.float32).reshape(-1), "flip_normals": np.ones(6, np.int32),
            "bsdf": np.zeros(6, np.int32), "emitter": np.zeros(6, np.int32), "radiance": RAD}


def _body_under_constant(scenes):
    """Scene B: the body alone under constant_environment(RAD)."""
    return {**_body(scenes), **scenes.constant_environment(RAD)}


# ---- a. the batch kernel --------------------------------------------------------
def test_env_eval_equals_host_bitwise(pkg, scenes, gpu):
    d, finite = ef.directions()
    dp = _planes(d, gpu)
    M = np.asarray(ef.ROTATIONS["cyc"], np.float32)
    cases = [ef.desc_of(px, scale, m) for _, px, scale in ef.maps() for m in (None, M)]
    cases.append(scenes.constant_environment(RAD))
    for i, env in enumerate(cases):
        sc = pkg.Scene({**_body(scenes), **env})
        got = np.stack([p.cpu().numpy() for p in sc.env_eval(dp)], -1)
        want = pkg.env_eval_host(env, d)
        assert np.array_equal(_bits(got), _bits(want)), i
        assert np.all(_bits(got[~finite]) == 0) or env["env_kind"] == 1
    # no environment: 0, whatever the direction
    none = pkg.Scene(_body_in_emitter_cube(scenes))
    got = np.stack([p.cpu().numpy() for p in none.env_eval(dp)], -1)
    assert np.all(_bits(got) == 0)


def test_scene_create_refuses_invalid_environments(pkg, scenes, gpu):
    """sdmm_scene_create validates the env fields as the host entry does."""
    px = ef.maps()[0][1]
    bad_px = px.copy()
    bad_px[1, 2, 0] = -1.0
    nan_m = np.eye(3, dtype=np.float32)
    nan_m[0, 0] = np.nan
    cases = [({"env_kind": 3}, "env_kind"), ({"env_kind": 2}, "env_pixels"),
             (ef.desc_of(bad_px), "texel"), (ef.desc_of(px, np.inf), "env_scale"),
             (ef.desc_of(px, 1.0, nan_m), "env_world_to_local"),
             ({"env_kind": 1, "env_radiance": [1.0, -2.0, 1.0]}, "env_radiance")]
    for env, word in cases:
        with pytest.raises(pkg.SDMMError, match="sdmm error -1") as e:
            pkg.Scene({**_body(scenes), **env})
        assert "sdmm_scene_create" in str(e.value) and word in str(e.value), str(e.value)
    # an environment does not change what geometry a scene must hold, nor its AABB
    with pytest.raises(pkg.SDMMError, match="sdmm error -1"):
        pkg.Scene({**_CAM, "reflectance": np.zeros(3, np.float32), **scenes.constant_environment(RAD)})
    plain = pkg.Scene(_body(scenes)).normalization()
    lit = pkg.Scene({**_body(scenes), **ef.desc_of(px)}).normalization()
    assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(plain, lit))


# ---- b. exact equivalence with emitter quads -------------------------------------
def _render_all(pkg, desc, gpu, **kw):
    import torch
    sc = pkg.Scene(desc)
    tree = _tree(pkg, sc)
    sqr = torch.zeros(3, sc.height, sc.width, device=gpu)
    img, verts, st = sc.render(tree, None, guided=False, image_sqr=sqr, **kw)
    rec, nv = verts.to_numpy()
    V = verts.s.max_vertices
    return img.cpu().numpy(), sqr.cpu().numpy(), rec.reshape(16, V, -1), nv, st


def test_constant_environment_equals_emitter_cube_bitwise(pkg, scenes, gpu):
    """A wall hit in A contributes thr * radiance through the same arithmetic
    as the environment in B and then dies on the wall's zero BSDF before saving
    a vertex; the random numbers are counter based.  Everything but the
    vertices' condition (fields 7-9: it depends on the scene AABB) is bitwise
    equal."""
    kw = dict(spp=4, max_depth=6, rr_depth=3, seed=6101)
    ia, sa, ra, nva, sta = _render_all(pkg, _body_in_emitter_cube(scenes), gpu, **kw)
    ib, sb, rb, nvb, stb = _render_all(pkg, _body_under_constant(scenes), gpu, **kw)
    assert np.array_equal(_bits(ia), _bits(ib))
    assert np.array_equal(_bits(sa), _bits(sb))
    assert np.array_equal(nva, nvb) and nva.max() >= 1 and (nva == 0).any()
    sel = np.arange(ra.shape[1])[:, None] < nva[None, :]
    for f in list(range(0, 7)) + list(range(10, 16)):
        assert np.array_equal(_bits(ra[f][sel]), _bits(rb[f][sel])), f
    assert np.any(ra[0][sel] != 0)                       # weights that the environment gave
    assert sta["paths"] == stb["paths"] and sta["segments"] == stb["segments"] > 0
    # the conditions do differ (another AABB): the excluded fields are not vacuous
    assert not np.array_equal(_bits(ra[7][sel]), _bits(rb[7][sel]))


# ---- c. known answers -------------------------------------------------------------
def test_constant_environment_known_answers(pkg, scenes, gpu):
    """BSDF only, one sample a pixel: a pixel whose camera ray misses the body
    is the radiance bitwise; a pixel on the body is rho x radiance (one bounce:
    no ray leaving the convex body meets it again)."""
    img, _, _, nv, st = _render_all(pkg, _body_under_constant(scenes), gpu, spp=1, max_depth=10, rr_depth=10, seed=6201)
    px = img.reshape(3, -1).T                            # [pixels, 3]
    miss = np.all(_bits(px) == _bits(RAD)[None, :], -1)
    body = np.all(np.abs(px.astype(np.float64) - RHO * RAD.astype(np.float64)) <= SLACK * RHO, -1)
    print(f"constant environment: {int(miss.sum())} pixels miss the body, {int(body.sum())} lie on it")
    assert np.all(miss ^ body)
    assert miss.sum() > 300 and body.sum() > 300
    grid = miss.reshape(36, 64)
    assert grid[0, 0] and grid[0, 63] and grid[35, 0] and grid[35, 63] and not grid[18, 32]
    assert np.array_equal(nv.reshape(36, 64) == 0, grid)   # a missing path saves no vertex
    assert st["segments"] == int(body.sum())


def _upper_half_map():
    """32x16: every row whose centre lies above the equator, plus the first row
    below it, is 1; the rest 0.  A direction with y >= 0 interpolates between
    texels that are all 1."""
    px = np.zeros((16, 32, 3), np.float32)
    px[:9] = 1.0
    return px


def test_upper_half_map_on_a_diffuse_quad(pkg, scenes, gpu):
    """A single upward-facing diffuse quad, rho 0.5, seen from above under the
    upper-half map: every bounce ray leaves upwards and sees 1, so every sample
    is rho (within the furnace test's margin), and so is the mean."""
    rho = 0.5
    desc = {"quads": np.asarray([-10.0, 0.0, -10.0, 0.0, 0.0, 20.0, 20.0, 0.0, 0.0], np.float32),
            "bsdf": np.zeros(1, np.int32), "reflectance": np.full(3, rho, np.float32),
            "camera_to_world": scenes._look_at((0.0, 2.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0)),
            "fov_x_deg": 60.0, "near_clip": 1e-2, "width": 64, "height": 36, **ef.desc_of(_upper_half_map())}
    img, _, _, nv, st = _render_all(pkg, desc, gpu, spp=1, max_depth=10, rr_depth=10, seed=6301)
    assert np.all(nv == 1) and st["segments"] == st["paths"]      # every camera ray meets the quad, once
    px = img.astype(np.float64)
    worst = float(np.abs(px - rho).max())
    print(f"upper-half map: mean {px.mean():.9f}, worst sample off by {worst:.3e} (margin {SLACK * rho:.3e})")
    assert worst <= SLACK * rho
    assert abs(px.mean() - rho) <= SLACK * rho
    # a delta lobe's bounce: the same quad as smooth plastic -- the mirror ray leaves upwards too, its radiance is
    # added (throughput x 1) and no vertex is saved (:764); the diffuse lobe saves one as before
    glossy = {**desc, "bsdf_params": scenes.plastic_params((rho, rho, rho))}
    pimg, _, _, pnv, pst = _render_all(pkg, glossy, gpu, spp=1, max_depth=10, rr_depth=10, seed=6302)
    lum = pimg.mean(0).reshape(-1)
    assert pst["segments"] == pst["paths"] and np.isfinite(lum).all() and np.all(lum > 0)
    assert (pnv == 0).sum() > 20 and (pnv == 1).sum() > 1000 and np.all(pnv <= 1)
    # the rows' orientation: with only the rows below those lit, the upward quad sees nothing
    lower = {**desc, "env_pixels": np.float32(1.0) - _upper_half_map()}
    dark = _render_all(pkg, lower, gpu, spp=1, max_depth=10, rr_depth=10, seed=6301)[0]
    assert float(np.abs(dark).max()) == 0.0


# ---- d. camera wiring with a varying map -------------------------------------------
def _rotation(axis, deg):
    a = np.asarray(axis, np.float64)
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.radians(deg)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def _smooth_map(scenes, w=16, h=8):
    """Low-order polynomials in the direction at the texel centres, positive."""
    uu, vv = np.meshgrid((np.arange(w) + 0.5) / w, (np.arange(h) + 0.5) / h)
    d = scenes.latlong_direction(uu, vv)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    return np.stack([1.5 + 0.7 * x + 0.5 * y * z, 1.2 + 0.6 * y - 0.4 * x * z, 1.0 + 0.5 * z + 0.3 * x * y + 0.2 * y * y],
                    -1).astype(np.float32)


def _camera_directions(oracle, desc, seed, dtype):
    """li_camera_kernel's mapping (spp 1: path = pixel) restated in numpy at
    `dtype`, the jitter from the oracle's rng_uniform."""
    T = dtype
    W, H = desc["width"], desc["height"]
    cam = desc["camera_to_world"].astype(T).reshape(4, 4)
    tanx = T(np.float32(np.tan(0.5 * float(desc["fov_x_deg"]) * 3.14159265358979323846 / 180.0)))
    aspect = T(np.float32(W) / np.float32(H))
    pix = np.arange(W * H)
    u0 = np.asarray([oracle.rng_uniform(seed, int(p), 0, 0) for p in pix], T)
    u1 = np.asarray([oracle.rng_uniform(seed, int(p), 0, 1) for p in pix], T)
    sx = ((pix % W).astype(T) + u0) / T(W)
    sy = ((pix // W).astype(T) + u1) / T(H)
    l = [(T(1) - T(2) * sx) * tanx, (T(1) - T(2) * sy) * tanx / aspect, np.ones(W * H, T)]
    inv = T(1) / np.sqrt(l[0] * l[0] + l[1] * l[1] + l[2] * l[2])
    l = [c * inv for c in l]
    d = [cam[r, 0] * l[0] + cam[r, 1] * l[1] + cam[r, 2] * l[2] for r in range(3)]
    dn = T(1) / np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    out = np.stack([c * dn for c in d], -1)
    assert out.dtype == T
    return out


def test_camera_rays_see_the_rotated_map(pkg, oracle, scenes, gpu, plog):
    """The body behind the camera: every camera ray misses, and each pixel is
    the lookup of its camera direction.  Bound: 4x the worst difference, pushed
    through the float64 lookup, between the float32 and the float64 restatement
    of the direction (9.99e-8 when this was written; the image's worst
    difference from env_eval_host of the float32 direction: 0)."""
    M = _rotation((1.0, 2.0, 3.0), 37.0)                  # the emitter's toWorld; the description takes its inverse
    px = _smooth_map(scenes)
    assert px.min() > 0.1
    env = ef.desc_of(px, 1.5, np.linalg.inv(M))
    desc = {**_body(scenes), **env, "camera_to_world": scenes._look_at((0.0, 0.3, 2.5), (0.4, 0.9, 6.0), (0.0, 1.0, 0.0))}
    seed = 6401
    img, _, _, nv, st = _render_all(pkg, desc, gpu, spp=1, max_depth=6, rr_depth=3, seed=seed)
    assert np.all(nv == 0) and st["segments"] == 0       # nothing is hit
    got = img.reshape(3, -1).T
    d32 = _camera_directions(oracle, desc, seed, np.float32)
    d64 = _camera_directions(oracle, desc, seed, np.float64)
    Minv = env["env_world_to_local"].reshape(3, 3)
    spread = float(np.abs(ef.restate(px, 1.5, Minv, d32, np.float64) - ef.restate(px, 1.5, Minv, d64, np.float64)).max())
    want = pkg.env_eval_host(env, d32)
    err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    print(f"camera wiring: image vs env_eval_host(float32 direction) {err:.3e}; float32 vs float64 direction through "
          f"the lookup {spread:.3e} (bound 4x = {4 * spread:.3e})")
    plog("env_camera_wiring_abs_err", err, 4 * spread, spread=spread)
    assert spread > 0
    assert err <= 4 * spread
    # the image varies: the map is seen, not a constant
    assert got.max() - got.min() > 0.2


# ---- e. guided renders of the open torus scene --------------------------------------
_CHILD = """
import sys
import numpy as np
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
from conftest import load_pkg
import importlib
pkg = load_pkg()
scenes = importlib.import_module("sdmm_mitsuba_amd.scenes")
from test_gpu_li import _tree
sc = pkg.Scene(scenes.torus_scene(160, 90, 24, 12, environment=scenes.sky_environment(64, 32)))
img = sc.render(_tree(pkg, sc), None, spp=8, guided=False, seed=4343)[0]
np.save({out!r}, img.cpu().numpy())
"""


@pytest.mark.parametrize("K", [16, 128])
def test_open_torus_scene(pkg, oracle, scenes, gpu, plog, K, tmp_path):
    import torch
    desc = scenes.torus_scene(160, 90, 24, 12, environment=scenes.sky_environment(64, 32))
    sc = pkg.Scene(desc)
    assert sc.n_triangles == 576 and sc.n_quads == 7
    tree = _tree(pkg, sc)
    node_mix = _train(pkg, sc, tree, 6, 8, K=K)
    assert any(m is not None for m in node_mix)
    B = len(desc["reflectance"]) // 3
    w, m, cov, dif = scenes.diffuse_learned_bsdf(B)
    table = pkg.BsdfTable(w, m, cov, device=gpu, diffuse=dif)
    spp = 64
    u_img, verts, _ = sc.render(tree, None, spp=spp, guided=False, seed=6151)
    u = _lum(u_img)
    assert np.isfinite(u).all() and u.mean() > 0
    for what, kw, seed in (("guided", {}, 6152), ("product", {"learned_bsdf": table}, 6153)):
        img, verts, st = sc.render(tree, node_mix, spp=spp, guided=True, seed=seed, **kw)
        g = _lum(img)
        assert np.isfinite(g).all() and st["guided_queries"] > 0
        s = plog(f"env_torus_{what}_K{K}_vs_unguided_sigma", _sigma(g, u), 4.0, guided=float(g.mean()),
                 unguided=float(u.mean()))
        assert s < 4.0, (what, g.mean(), u.mean())
    if K != 16:
        return
    # the scene has no other emitter: every non-zero vertex weight came from the environment
    img, verts, _ = sc.render(tree, node_mix, spp=4, guided=True, seed=6154)
    first = img.clone()
    rec, nv = verts.to_numpy()
    r = rec.reshape(16, verts.s.max_vertices, -1)
    sel = np.arange(r.shape[1])[:, None] < nv[None, :]
    lit = (r[0][sel] != 0) | (r[1][sel] != 0) | (r[2][sel] != 0)
    print(f"saved vertices with a weight from the environment: {int(lit.sum())} of {lit.size} ({100 * lit.mean():.1f} %)")
    assert int(lit.sum()) > 0
    _check_producer(pkg, oracle, tree, verts, 8, 0xE57, plog, "env_torus_guided")
    # the same seed renders the same image
    again = sc.render(tree, node_mix, spp=4, guided=True, seed=6154)[0]
    assert torch.equal(first, again)
    # the brute-force loop (SDMM_MESH_BRUTE=1, read at scene creation) in a fresh process
    bvh = sc.render(tree, None, spp=8, guided=False, seed=4343)[0].cpu().numpy()
    out = tmp_path / "brute.npy"
    script = tmp_path / "brute_child.py"
    script.write_text(_CHILD.format(root=str(ROOT), tests=str(ROOT / "tests"), out=str(out)))
    r = subprocess.run([sys.executable, str(script)], env={**os.environ, "SDMM_MESH_BRUTE": "1"}, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.array_equal(np.load(out).view(np.uint32), bvh.view(np.uint32))


# ---- f. no regression ---------------------------------------------------------------
def test_env_kind_zero_renders_the_same(pkg, scenes, gpu):
    """env_kind = 0 with arbitrary values in the other env fields: bitwise the
    image of the description without those keys, unguided and guided."""
    import torch
    plain = scenes.cornell_box(64, 36)
    with_fields = {**plain, "env_kind": 0, "env_radiance": np.asarray([5.0, np.nan, -1.0], np.float32),
                   "env_pixels": np.full((4, 8, 3), -7.0, np.float32), "env_scale": float("inf"),
                   "env_world_to_local": np.full(9, np.nan, np.float32)}
    a, b = pkg.Scene(plain), pkg.Scene(with_fields)
    tree = _tree(pkg, a)
    node_mix = _train(pkg, a, tree, 4, 8, K=16)
    assert any(m is not None for m in node_mix)
    for guided in (False, True):
        ia, _, sa = a.render(tree, node_mix if guided else None, spp=2, guided=guided, seed=6501)
        ia = ia.clone()
        ib, _, sb = b.render(tree, node_mix if guided else None, spp=2, guided=guided, seed=6501)
        assert torch.equal(ia, ib) and sa == sb
        assert not guided or sa["guided_queries"] > 0
