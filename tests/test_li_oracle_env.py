"""CPU: the oracle's environment emitters (oracle/sdmm_oracle_li.inc:
li_env_eval, the two escape points of li_path, the `escaped` output) -- what
the device Li's environment is compared with in
tests/test_gpu_li_oracle_env.py -- shown right on their own:

  * oracle.env_eval against the float64 numpy restatement on the fixture's
    maps and directions (tests/env_fixture.py), within 4x the float32
    restatement's own worst error; non-finite directions 0; a constant
    emitter its radiance bitwise;
  * oracle.env_eval == pkg.env_eval_host bit for bit: two texts written
    separately from envmap.cpp / mipmap.h (the oracle's in C from the
    reference, the library's csrc/envmap.h) keep the same operation order;
  * the oracle's Li: a constant environment equals a closed cube of emitter
    quads path for path, the upper-half map lights an upward quad to rho and
    its complement to 0, `escaped` row 0 marks the camera rays that left;
  * the map of the guided GPU cases moves by less than _compare_guided's
    record tolerance under a 1e-5 move of the direction -- the sky map does
    not (the sun disc's edge), so it serves the bit-exact cases alone."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import env_fixture as ef  # noqa: E402
from test_gpu_env import (RAD, SLACK, _body_in_emitter_cube, _body_under_constant, _rotation, _smooth_map,  # noqa: E402
                          _upper_half_map)

LEAF = (np.float32([[0, 0, 0, 1, 1, 1]]), np.int32([[-1, -1]]))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the environments of tests/test_gpu_li_oracle_env.py ---------------------------
def env_rotation():
    """The emitters' toWorld: 37 degrees about (1, 2, 3) -- no signed
    permutation, so every product of the world-to-local transform rounds."""
    return _rotation((1.0, 2.0, 3.0), 37.0)


def sky_env(scenes):
    """sky_environment(64, 32), rotated: for the bit-exact cases."""
    return scenes.sky_environment(64, 32, to_world=env_rotation())


def smooth_env(scenes, w=64, h=32):
    """The polynomials of test_gpu_env._smooth_map at w x h, rotated, scale
    1.5: the guided cases' map."""
    return ef.desc_of(_smooth_map(scenes, w, h), 1.5, np.linalg.inv(env_rotation()))


def _cases():
    """(name, pixels, scale, world-to-local or None): the fixture's five sizes, identity and `cyc`."""
    cyc = np.asarray(ef.ROTATIONS["cyc"], np.float32)
    return [(f"{name}-{tag}", px, scale, M) for name, px, scale in ef.maps() for tag, M in (("id", None), ("cyc", cyc))]


# ---- oracle.env_eval ------------------------------------------------------------------
@pytest.mark.parametrize("which", range(10))
def test_env_eval_against_float64_restatement(oracle, plog, which):
    """tests/test_env.py's rule: every finite direction within 4x the worst
    error of the numpy float32 restatement against the float64 one on the same
    inputs -- the float32 restatement's rounding is the only error source.
    Realised (oracle / float32 restatement): 8x4 6.81e-7 / 6.81e-7 and 6.66e-7 /
    6.66e-7 (cyc); 16x8 1.00e-6 / 1.00e-6 and 1.12e-6 / 9.09e-7; 1x1 2.38e-7 /
    2.38e-7 both; 1x4 4.50e-7 / 4.14e-7 and 4.85e-7 / 4.17e-7; 4x1 4.72e-7 /
    4.72e-7 and 5.61e-7 / 4.17e-7."""
    name, px, scale, M = _cases()[which]
    d, finite = ef.directions()
    got = oracle.env_eval(ef.desc_of(px, scale, M), d)
    assert got.shape == (len(d), 3) and got.dtype == np.float32
    r64 = ef.restate(px, scale, M, d[finite], np.float64)
    r32 = ef.restate(px, scale, M, d[finite], np.float32)
    err32 = float(np.abs(r32.astype(np.float64) - r64).max())
    err = float(np.abs(got[finite].astype(np.float64) - r64).max())
    print(f"oracle env {name}: {err:.3e}, numpy float32 restatement {err32:.3e} (bound 4x = {4 * err32:.3e})")
    plog(f"oracle_env_eval_{name}_abs_err", err, 4 * err32)
    assert err32 > 0
    assert err <= 4 * err32
    if px.shape[0] * px.shape[1] > 1:                    # the map is seen, not one value
        assert got[finite].max() > 0.8 * scale * px.max() and got[finite].min() < 1.5 * scale * px.min()


def test_env_eval_nonfinite_and_constant(oracle, scenes):
    d, finite = ef.directions()
    assert (~finite).sum() == 2
    for name, px, scale, M in _cases():
        got = oracle.env_eval(ef.desc_of(px, scale, M), d)
        assert np.all(_bits(got[~finite]) == 0), name
        assert np.all(got[finite] > 0), name
    got = oracle.env_eval(scenes.constant_environment(RAD), d)
    assert np.all(_bits(got) == _bits(RAD)[None, :])
    # a constant emitter reads neither scale nor transform nor map; no emitter: 0
    noisy = {**scenes.constant_environment(RAD), "env_scale": np.nan, "env_world_to_local": np.full(9, np.inf)}
    assert np.all(_bits(oracle.env_eval(noisy, d)) == _bits(RAD)[None, :])
    assert np.all(_bits(oracle.env_eval({"env_kind": 0, "env_radiance": RAD}, d)) == 0)
    assert np.all(_bits(oracle.env_eval({}, d)) == 0)


def test_env_eval_equals_host_bitwise(pkg, oracle, scenes):
    """The oracle's C text and csrc/envmap.h, written separately, agree bit for
    bit: on the fixture's maps and directions (identity and cyc), a constant
    emitter, and the two rotated 64x32 maps of the GPU cases."""
    d, _ = ef.directions()
    envs = [(name, ef.desc_of(px, scale, M)) for name, px, scale, M in _cases()]
    envs += [("constant", scenes.constant_environment(RAD)), ("sky", sky_env(scenes)), ("smooth", smooth_env(scenes))]
    for name, env in envs:
        a, b = oracle.env_eval(env, d), pkg.env_eval_host(env, d)
        differ = int((_bits(a) != _bits(b)).any(-1).sum())
        assert differ == 0, (name, differ, float(np.nanmax(np.abs(a - b))))


# ---- the oracle's Li -----------------------------------------------------------------
def test_constant_environment_equals_emitter_cube_bitwise(oracle, scenes):
    """tests/test_gpu_env.py's pair on the oracle alone: a wall hit in the
    closed emitter cube contributes thr * radiance as the environment does and
    the path ends on the wall's zero BSDF; image, nv and every record field
    but the condition (7-9: another scene box) are equal bit for bit."""
    kw = dict(spp=4, max_depth=6, rr_depth=3, seed=6101, threads=4)
    a = oracle.li_render(_body_in_emitter_cube(scenes), *LEAF, **kw)
    b = oracle.li_render(_body_under_constant(scenes), *LEAF, **kw)
    assert np.array_equal(_bits(a["image"]), _bits(b["image"]))
    assert np.array_equal(_bits(a["image_sqr"]), _bits(b["image_sqr"]))
    assert np.array_equal(a["nv"], b["nv"]) and a["nv"].max() >= 1 and (a["nv"] == 0).any()
    sel = np.arange(a["rec"].shape[1])[:, None] < a["nv"][None, :]
    for f in list(range(0, 7)) + list(range(10, 16)):
        assert np.array_equal(_bits(a["rec"][f][sel]), _bits(b["rec"][f][sel])), f
    assert np.any(a["rec"][0][sel] != 0)
    assert not np.array_equal(_bits(a["rec"][7][sel]), _bits(b["rec"][7][sel]))
    # the closed cube lets no ray out; under the environment every ray the cube's walls caught leaves
    assert not (a["escaped"] == 1).any() and (b["escaped"] == 1).any()
    assert np.array_equal(a["escaped"] == -1, b["escaped"] == -1)
    assert np.array_equal(a["comps"], b["comps"]) and np.array_equal(a["hit_bsdf"], b["hit_bsdf"])


def test_escaped_row_zero_marks_the_camera_rays_that_left(oracle, scenes):
    """One sample a pixel (path = pixel) of the body under the constant
    environment: escaped row 0 is 1 exactly where no vertex was saved and the
    image is non-zero -- there the pixel is the radiance bitwise; elsewhere it
    is 0 (the ray hit the body) and the bounce's ray left (row 1)."""
    r = oracle.li_render(_body_under_constant(scenes), *LEAF, spp=1, max_depth=10, rr_depth=10, seed=6201)
    px = r["image"].reshape(3, -1).T
    lit = (px != 0).any(-1)
    esc = r["escaped"]
    assert esc.shape == (10, px.shape[0]) and esc.dtype == np.int32
    assert np.array_equal(esc[0] == 1, (r["nv"] == 0) & lit)
    assert np.array_equal(esc[0] == 0, r["nv"] >= 1) and not (esc[0] == -1).any()
    assert (esc[0] == 1).sum() > 300 and (esc[0] == 0).sum() > 300
    assert np.all(_bits(px[esc[0] == 1]) == _bits(RAD)[None, :])
    # a convex body: the one bounce ray of a path that hit it leaves; no further ray
    assert np.array_equal(esc[1] == 1, esc[0] == 0) and np.all(esc[1][esc[0] == 1] == -1)
    assert np.all(esc[2:] == -1)


def test_upper_half_map_on_a_diffuse_quad(oracle, scenes):
    """tests/test_gpu_env.py's known answer on the oracle: an upward diffuse
    quad under the upper-half map returns rho in every sample, 0 under the
    complement; as smooth plastic a delta bounce adds radiance without a vertex."""
    rho = 0.5
    desc = {"quads": np.asarray([-10.0, 0.0, -10.0, 0.0, 0.0, 20.0, 20.0, 0.0, 0.0], np.float32),
            "bsdf": np.zeros(1, np.int32), "reflectance": np.full(3, rho, np.float32),
            "camera_to_world": scenes._look_at((0.0, 2.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0)),
            "fov_x_deg": 60.0, "near_clip": 1e-2, "width": 64, "height": 36, **ef.desc_of(_upper_half_map())}
    assert "radiance" not in desc and "emitter" not in desc          # an open scene has no other light
    r = oracle.li_render(desc, *LEAF, spp=1, max_depth=10, rr_depth=10, seed=6301)
    assert np.all(r["nv"] == 1) and np.all(r["escaped"][0] == 0) and np.all(r["escaped"][1] == 1)
    px = r["image"].astype(np.float64)
    assert float(np.abs(px - rho).max()) <= SLACK * rho
    lower = {**desc, "env_pixels": np.float32(1.0) - _upper_half_map()}
    dark = oracle.li_render(lower, *LEAF, spp=1, max_depth=10, rr_depth=10, seed=6301)
    assert float(np.abs(dark["image"]).max()) == 0.0 and np.all(dark["escaped"][1] == 1)
    glossy = {**desc, "bsdf_params": scenes.plastic_params((rho, rho, rho))}
    p = oracle.li_render(glossy, *LEAF, spp=1, max_depth=10, rr_depth=10, seed=6302)
    lum = p["image"].mean(0).reshape(-1)
    assert np.isfinite(lum).all() and np.all(lum > 0) and np.all(p["escaped"][1] == 1)
    assert (p["nv"] == 0).sum() > 20 and (p["nv"] == 1).sum() > 1000 and np.all(p["nv"] <= 1)


def test_threads_and_absent_fields_do_not_change_results(oracle, scenes):
    """env_kind = 0 with arbitrary values in the other env fields renders as
    the description without them; threads do not change an open scene's result."""
    plain = scenes.cornell_box(32, 18)
    with_fields = {**plain, "env_kind": 0, "env_radiance": np.asarray([5.0, np.nan, -1.0], np.float32),
                   "env_pixels": np.full((4, 8, 3), -7.0, np.float32), "env_scale": float("inf"),
                   "env_world_to_local": np.full(9, np.nan, np.float32)}
    a = oracle.li_render(plain, *LEAF, spp=2, seed=31)
    b = oracle.li_render(with_fields, *LEAF, spp=2, seed=31)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    desc = scenes.torus_scene(32, 18, 24, 12, environment=sky_env(scenes))
    a = oracle.li_render(desc, *LEAF, spp=2, rr_depth=3, seed=3, threads=1)
    b = oracle.li_render(desc, *LEAF, spp=2, rr_depth=3, seed=3, threads=5)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    # (the camera looks down at the floor: its rays all hit; the bounce rays leave)
    assert np.all(a["escaped"][0] == 0) and (a["escaped"][1:] == 1).sum() > 20


# ---- which map the guided cases can use ------------------------------------------------
def _sensitivity(env, n=200_000, step=1e-5, seed=20241022):
    """The float64 lookup at n random unit directions and at each moved by
    `step` (along a random unit tangent, renormalised): the worst change over
    _compare_guided's record tolerance (1e-5 + 1e-3 |value|), and the fraction
    of directions over it."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    t = np.cross(d, rng.normal(size=(n, 3)))
    t /= np.linalg.norm(t, axis=-1, keepdims=True)
    e = d + step * t
    e /= np.linalg.norm(e, axis=-1, keepdims=True)
    px, scale, M = env["env_pixels"], env["env_scale"], env["env_world_to_local"]
    a, b = ef.restate(px, scale, M, d, np.float64), ef.restate(px, scale, M, e, np.float64)
    ratio = (np.abs(b - a) / (1e-5 + 1e-3 * np.abs(a))).max(-1)
    return float(ratio.max()), float((ratio > 1.0).mean())


def test_guided_cases_map_is_insensitive_to_the_guide_direction_rounding(scenes, plog):
    """The guide's direction differs by up to 1e-5 between device and oracle
    (tests/test_gpu_parity.py); the escape value env(wo) enters the records
    through value / clampedPdf and thr * value.  The smooth 64x32 map moves by
    well under the record tolerance (worst 0.08 of it when this was written,
    0.29 at 16x8); the sky map's sun-disc edge moves by 64x the tolerance on
    0.05 % of the directions, so it stays with the bit-exact cases."""
    worst, over = _sensitivity(smooth_env(scenes))
    plog("env_smooth_64x32_change_over_record_tolerance", worst, 1.0, directions_over=over)
    assert worst < 1.0 and over == 0.0, (worst, over)
    coarse, over16 = _sensitivity(smooth_env(scenes, 16, 8))
    sky, over_sky = _sensitivity(sky_env(scenes))
    print(f"1e-5 move / record tolerance: smooth 64x32 {worst:.3f}, smooth 16x8 {coarse:.3f} ({over16:.2%} over), "
          f"sky 64x32 {sky:.1f} ({over_sky:.3%} over)")
    assert coarse < 1.0 and over16 == 0.0
    assert sky > 1.0 and over_sky > 0.0                  # why the sky map is not used there
