"""GPU: the environment emitter of the device Li (the ENV variants of
li_camera_kernel and li_shade_kernel, csrc/render.hip: env(d) for a camera ray
that hits nothing, value = env(wo) for a bounce ray that hits nothing, thr *
value into the path, record_radiance into every earlier vertex, value /
clampedPdf as the new vertex's weight) against the CPU restatement
(oracle/sdmm_oracle_li.inc, pinned on its own in tests/test_li_oracle_env.py),
path by path, in the forms of tests/test_gpu_li_oracle.py: unguided bit-exact
-- also with Russian roulette on -- guided and product through _compare_guided,
unchanged.

The maps vary with the direction and are rotated by a matrix that is no signed
permutation, so a wrong vector (d for wo, a local-frame vector, a missed
env_world_to_local) or a stale value changes records and image.  The lookup
adds no device transcendental that Scene.env_eval == env_eval_host
(tests/test_gpu_env.py) does not already hold bitwise: zero mismatching paths,
no exclusions.

Which scene launches which kernel (all with ENV = true):

  li_shade_kernel<PHONG, DIEL, MESH>      scene
  <false, false, false>                   open Cornell: plain, plastic floor
  <true,  false, false>                   open Cornell, Phong tall box and floor
  <false, true,  false>                   open Cornell, glass tall box
  <true,  true,  false>                   open Cornell, Phong short box and floor, glass tall box
  <false, false, true >                   open Cornell, both cubes as triangles
  <true,  false, true >                   open Cornell, cubes as triangles, Phong floor
  <false, true,  true >                   open torus scene (glass case of quads, torus mesh)
  <true,  true,  true >                   open torus scene with a Phong floor
  li_camera_kernel<MESH = false>          the open Cornell scenes without a mesh
  li_camera_kernel<MESH = true>           the open Cornell with cubes as triangles, the torus scenes

Every case counts, from the oracle's outputs alone (escaped / comps / hit_bsdf
/ inside / rec / nv), that its paths met the code it is about, and asserts
each count with a margin of at least 2x under what the oracle gave when this
was written (GUARDS)."""
import numpy as np
import pytest

from test_gpu_li_oracle import SEED, SPP, _compare_guided
from test_gpu_li_oracle_dielectric import _assert_bitwise, _glass_box, _guided, _roulette_deaths, _unguided
from test_li_oracle_env import sky_env, smooth_env

pytestmark = pytest.mark.gpu

W, H = 128, 72
P = W * H * SPP
CUBES = ("ShortBox", "TallBox")
TORUS_NAMES = ["Room", "Floor", "Torus", "Glass", "Light"]


def _ids(scenes, names):
    return [list(scenes._BSDFS).index(n) for n in names]


def _open(scenes, desc):
    """A Cornell box description without its ceiling, its back wall and its
    lamp: the rows of those quads dropped.  No emitter quad is left."""
    gone = _ids(scenes, ("Ceiling", "BackWall", "Light"))
    keep = ~np.isin(desc["bsdf"], gone)
    out = dict(desc)
    out["quads"] = np.ascontiguousarray(desc["quads"].reshape(-1, 9)[keep].reshape(-1))
    for k in ("flip_normals", "bsdf", "emitter"):
        out[k] = np.ascontiguousarray(desc[k][keep])
    assert keep.sum() == len(keep) - 3 and np.all(out["emitter"] == -1)
    return out


def _torus_floor_phong(scenes, desc):
    bp = desc["bsdf_params"].reshape(-1, 8).copy()
    refl = desc["reflectance"].reshape(-1, 3).copy()
    f = TORUS_NAMES.index("Floor")
    bp[f], refl[f] = scenes.phong_params(tuple(refl[f]), (0.4, 0.4, 0.4), 30.0)
    return {**desc, "bsdf_params": bp.reshape(-1), "reflectance": refl.reshape(-1)}


def _scene(scenes, case, env, alpha=None, fov=None):
    """(description, {"phong": ids, "glass": ids, "plastic": ids}) of a case
    under the environment env.  alpha: another Beckmann alpha for the glass;
    fov: another horizontal field of view for the open Cornell's camera."""
    ids = {"phong": [], "glass": [], "plastic": []}
    if case.startswith("torus"):
        desc = scenes.torus_scene(W, H, 24, 12, environment=env)
        ids["glass"] = [TORUS_NAMES.index("Glass")]
        if alpha is not None:
            bp = desc["bsdf_params"].reshape(-1, 8).copy()
            bp[ids["glass"][0], 6] = alpha
            desc["bsdf_params"] = bp.reshape(-1)
        if case == "torus_phong":
            desc = _torus_floor_phong(scenes, desc)
            ids["phong"] = [TORUS_NAMES.index("Floor")]
        assert np.all(desc["emitter"] == -1)
        return desc, ids
    kw = {"plain": {}, "plastic": dict(plastic=("Floor",)), "phong": dict(phong=("TallBox", "Floor")),
          "glass": dict(dielectric=("TallBox",)),
          "phong_glass": dict(phong=("ShortBox", "Floor"), dielectric=("TallBox",)),
          "mesh": dict(mesh=CUBES), "phong_mesh": dict(mesh=CUBES, phong=("Floor",))}[case]
    if "dielectric" in kw:
        desc = _glass_box(scenes, W, H, dielectric_alpha=0.1 if alpha is None else alpha, **kw)   # lifted off the floor
    else:
        desc = scenes.cornell_box(W, H, **kw)
    for k, key in (("phong", "phong"), ("glass", "dielectric"), ("plastic", "plastic")):
        ids[k] = _ids(scenes, kw.get(key, ()))
    if fov is not None:
        desc["fov_x_deg"] = fov
    return {**_open(scenes, desc), **env}, ids


def _guard_counts(r, ids):
    """From the oracle's outputs alone.  A path has at most one escaping
    bounce ray, its last.  Where every traced ray of a path saved a vertex
    (rays == nv: no delta lobe on the way; V = 9 covers every bounce), saved
    vertex v is bounce v.  The scenes hold no emitter quad, so a non-zero
    weight (fields 0-2) comes from an escape: at the escaping bounce's own
    vertex value / clampedPdf, at an earlier vertex record_radiance."""
    esc = r["escaped"][1:] == 1                               # [bounces, P]
    B, n = esc.shape
    assert (esc.sum(0) <= 1).all()
    has = esc.any(0)
    eb = esc.argmax(0)                                        # the escaping bounce
    rays = (r["escaped"][1:] >= 0).sum(0)
    nv = r["nv"]
    assert (rays >= nv).all() and (np.where(has, eb == rays - 1, True)).all()
    nz = (r["rec"][0:3] != 0).any(0)                          # [V, P]
    V = nz.shape[0]
    assert V >= B
    plain = has & (rays == nv)                                # vertex v is bounce v
    col = np.arange(n)
    own = plain & nz[np.minimum(eb, V - 1), col]
    earlier = (nz & (np.arange(V)[:, None] < eb[None, :]) & plain[None, :]).sum()
    at = lambda a: a[eb, col]                                 # a per-bounce array at the escaping bounce
    # a delta lobe's escape, counted where it cannot be mistaken: the path's only plastic bounce is its last
    # ray and exactly one ray saved no vertex
    on_plastic = np.isin(r["hit_bsdf"], ids["plastic"])
    delta = has & at(on_plastic) & (on_plastic.sum(0) == 1) & (rays - nv == 1)
    return {"camera_escapes": int((r["escaped"][0] == 1).sum()),
            "escapes_depth1": int(esc[0].sum()),
            "escapes_depth2plus": int(esc[1:].sum()),
            "escape_weights_nonzero": int(own.sum()),
            "earlier_vertices_lit": int(earlier),
            "escapes_after_delta": int(delta.sum()),
            "escapes_from_inside_glass": int((has & (at(r["inside"]) == 1)
                                              & at(np.isin(r["hit_bsdf"], ids["glass"]))).sum()),
            "escapes_after_phong": int((has & at(np.isin(r["hit_bsdf"], ids["phong"]))).sum()),
            "escapes_guide_sampled": int((has & (at(r["comps"]) >= 0)).sum())}


def _check_guards(plog, tag, counts, minima):
    print(f"{tag} guards: {counts}")
    for k, least in minima.items():
        plog(f"{tag}_{k}", counts[k], least, lower=True)
        assert counts[k] >= least, (tag, k, counts[k], least)


# Lower bounds, each at most half of what the oracle counted when this was written
# (profiles/env_oracle_parity_errors.jsonl holds the counts of the committed run).
_CORNELL = {"camera_escapes": 10000, "escapes_depth1": 2000, "escapes_depth2plus": 2000, "escape_weights_nonzero": 4000,
            "earlier_vertices_lit": 4000}
_TORUS = {"escapes_depth1": 1000, "escapes_depth2plus": 10000, "escape_weights_nonzero": 10000,
          "earlier_vertices_lit": 40000, "escapes_from_inside_glass": 10000}
# (the torus scenes' camera looks down at the floor and none of its rays leaves: li_camera_kernel<MESH = true>'s
# escape is held by the open Cornell with its cubes as triangles)
GUARDS = {
    "plain": _CORNELL,
    "plastic": {**_CORNELL, "escapes_after_delta": 150},
    "phong": {**_CORNELL, "escapes_after_phong": 1500},
    "glass": {**_CORNELL, "escapes_from_inside_glass": 1000},
    "phong_glass": {**_CORNELL, "escapes_from_inside_glass": 1000, "escapes_after_phong": 1200},
    "mesh": _CORNELL,
    "phong_mesh": {**_CORNELL, "escapes_after_phong": 800},
    "torus": _TORUS,
    "torus_phong": {**_TORUS, "escapes_after_phong": 2000},
}
GUARDS_CONSTANT = _CORNELL
GUARDS_RR = {
    "plain": {"camera_escapes": 10000, "escapes_depth1": 2000, "escapes_depth2plus": 1200, "escape_weights_nonzero": 3000,
              "earlier_vertices_lit": 1500, "roulette_deaths": 1000, "escapes_after_roulette": 300},
    "glass": {"camera_escapes": 10000, "escapes_depth1": 2000, "escapes_depth2plus": 1500, "escape_weights_nonzero": 3000,
              "earlier_vertices_lit": 2500, "escapes_from_inside_glass": 1000, "roulette_deaths": 800,
              "escapes_after_roulette": 500},
}
GUARDS_GUIDED = {     # the least of the guided and product runs (and of K = 16 and 128), halved
    "plain": {"camera_escapes": 9000, "escapes_depth1": 6000, "escapes_depth2plus": 2800, "escape_weights_nonzero": 8500,
              "earlier_vertices_lit": 4500, "escapes_guide_sampled": 5000},
    "torus": {"escapes_depth1": 5000, "escapes_depth2plus": 4000, "escape_weights_nonzero": 11000,
              "earlier_vertices_lit": 11000, "escapes_from_inside_glass": 3500, "escapes_guide_sampled": 7000},
}


@pytest.mark.parametrize("case", ["plain", "plastic", "phong", "glass", "phong_glass", "mesh", "phong_mesh", "torus",
                                  "torus_phong"])
def test_open_scene_unguided_bitwise(pkg, oracle, scenes, gpu, plog, case):
    """Every scene under the rotated sky map: nv, every live record field and
    the image bit for bit."""
    desc, ids = _scene(scenes, case, sky_env(scenes))
    img, rec, nv, r, _ = _unguided(pkg, oracle, desc)
    assert nv.shape[0] == P
    tag = f"li_env_{case}_sky_unguided"
    c = _guard_counts(r, ids)
    _check_guards(plog, tag, c, GUARDS[case])
    _assert_bitwise(plog, tag, img, rec, nv, r, **c)


def test_open_cornell_constant_unguided_bitwise(pkg, oracle, scenes, gpu, plog):
    desc, ids = _scene(scenes, "plain", scenes.constant_environment((1.0, 0.8, 0.6)))
    img, rec, nv, r, _ = _unguided(pkg, oracle, desc)
    c = _guard_counts(r, ids)
    _check_guards(plog, "li_env_plain_constant_unguided", c, GUARDS_CONSTANT)
    _assert_bitwise(plog, "li_env_plain_constant_unguided", img, rec, nv, r, **c)


@pytest.mark.parametrize("case", ["plain", "glass"])
def test_open_cornell_roulette_bitwise(pkg, oracle, scenes, gpu, plog, case):
    """rr_depth = 2: the roulette is drawn only when the ray hit something
    (alive = q >= 0), so an escaping ray consumes no draw and is not rescaled;
    survivors' later escapes carry thr / q."""
    desc, ids = _scene(scenes, case, sky_env(scenes))
    img, rec, nv, r, (aabb, child) = _unguided(pkg, oracle, desc, rr_depth=2)
    r10 = oracle.li_render(desc, aabb, child, spp=SPP, seed=SEED, threads=16)
    c = _guard_counts(r, ids)
    c["roulette_deaths"] = _roulette_deaths(r, r10)
    # escapes at a depth the roulette had already rescaled the throughput at
    c["escapes_after_roulette"] = int((r["escaped"][3:] == 1).sum())
    tag = f"li_env_{case}_sky_rr2_unguided"
    _check_guards(plog, tag, c, GUARDS_RR[case])
    _assert_bitwise(plog, tag, img, rec, nv, r, **c)


@pytest.mark.parametrize("case,K,product", [("plain", 16, False), ("plain", 16, True), ("torus", 16, False),
                                            ("torus", 16, True), ("plain", 128, False), ("plain", 128, True)],
                         ids=["plain-K16-guided", "plain-K16-product", "torus-K16-guided", "torus-K16-product",
                              "plain-K128-guided", "plain-K128-product"])
def test_open_scene_guided_li_matches_oracle(pkg, oracle, scenes, gpu, plog, case, K, product):
    """Guided and product bounces under the smooth map (the sky map's sun-disc
    edge is too sensitive to the guide direction's last digits:
    tests/test_li_oracle_env.py).  The torus scene's case at alpha 0.3, for the
    reason given in tests/test_gpu_li_oracle_mesh.py.  The open Cornell at a
    field of view of 20 degrees, not 35: the camera stands well outside the box,
    and with the back wall gone 72 % of the 35 degree view's rays leave at once,
    too few bounces left for _compare_guided's own guard (guide samples > P / 4);
    at 20 degrees half the camera rays still leave."""
    desc, ids = _scene(scenes, case, smooth_env(scenes), alpha=0.3 if case == "torus" else None,
                       fov=20.0 if case == "plain" else None)
    img, rec, nv, r = _guided(pkg, oracle, scenes, gpu, desc, K, product=product)
    tag = f"li_env_{case}_smooth_K{K}_{'product' if product else 'guided'}"
    c = _guard_counts(r, ids)
    _check_guards(plog, tag, c, GUARDS_GUIDED[case])
    _compare_guided(oracle, plog, tag, img, rec, nv, r)
