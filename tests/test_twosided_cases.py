"""CPU: the `twosided` adapter's description field and the scenes its GPU
tests stand on (include/sdmm_gpu.h sdmm_scene_desc.bsdf_twosided).

  * validation through sdmm_scene_intersect_host, which validates a
    description as sdmm_scene_create does: an entry other than 0 or 1 and a 1
    on a transmitting BSDF (kinds 4 and 5) are SDMM_E_INVALID with a message;
    no table and all zeros pass;
  * scenes.mirror_z is exact: the mirror twin's rays hit the same primitives
    at bitwise the same distance -- what test_gpu_twosided.py's bitwise twin
    test stands on, checked where no GPU is needed;
  * scenes.sheet_scene: no zero-area triangle, host BVH == brute loop bitwise
    on its camera rays, and between 30 % and 70 % of the camera rays that hit
    the sheet meet its back (a condition on the scene, tuned there).
"""
import numpy as np
import pytest

import twosided_fixture as tf


def _expect_invalid(pkg, desc, match):
    o, d = np.zeros((1, 3), np.float32), np.array([[0.0, 0.0, 1.0]], np.float32)
    # SDMM_E_INVALID = -1, with the message naming the fault
    with pytest.raises(pkg.SDMMError, match=r"sdmm error -1: sdmm_scene_intersect_host: .*" + match):
        pkg.intersect_host(desc, o, d)


def test_bsdf_twosided_is_validated(pkg, scenes):
    base = scenes.cornell_box(16, 9, dielectric=("TallBox",), glass=("ShortBox",), mirror=("Floor",))
    names = list(scenes._BSDFS)
    B = len(names)
    o, d = tf.camera_rays(base)
    want = pkg.intersect_host(base, o, d)
    # no table, all zeros, and ones on non-transmitting kinds (0 and 6 here) pass
    ok = np.zeros(B, np.int32)
    for flags in (None, ok, np.asarray([int(nm in ("Floor", "LeftWall", "Light")) for nm in names], np.int32)):
        got = pkg.intersect_host({**base, "bsdf_twosided": flags}, o, d)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    for bad in (2, -1):
        flags = ok.copy()
        flags[names.index("LeftWall")] = bad
        _expect_invalid(pkg, {**base, "bsdf_twosided": flags}, "bsdf_twosided entry other than 0 or 1")
    for nm in ("TallBox", "ShortBox"):                      # kinds 4 and 5
        flags = ok.copy()
        flags[names.index(nm)] = 1
        assert base["bsdf_params"][8 * names.index(nm)] in (4.0, 5.0)
        _expect_invalid(pkg, {**base, "bsdf_twosided": flags}, "bsdf_twosided on a transmitting BSDF")
    # the builders refuse the same names
    with pytest.raises(ValueError, match="twosided"):
        scenes.cornell_box(16, 9, glass=("ShortBox",), twosided=("ShortBox",))
    with pytest.raises(ValueError, match="twosided"):
        scenes.cornell_box(16, 9, twosided=("NoSuchBsdf",))
    # one entry per BSDF
    with pytest.raises(pkg.SDMMError, match="one entry per BSDF"):
        pkg.intersect_host({**base, "bsdf_twosided": np.zeros(B + 1, np.int32)}, o, d)
    flagged = scenes.cornell_box(16, 9, twosided=("Floor", "TallBox"))
    assert flagged["bsdf_twosided"].tolist() == [int(nm in ("Floor", "TallBox")) for nm in names]
    assert "bsdf_twosided" not in scenes.cornell_box(16, 9)


@pytest.mark.parametrize("kind", [0, 3])
def test_mirror_z_is_exact(pkg, scenes, kind):
    A, B = tf.twin_scenes(scenes, kind)
    qa, qb = A["quads"].reshape(-1, 3, 3), B["quads"].reshape(-1, 3, 3)
    assert np.array_equal(qa[..., :2], qb[..., :2]) and np.array_equal(qa[..., 2], -qb[..., 2])
    assert B["flip_normals"].tolist() == [0] * 6 + [0] and A["flip_normals"].tolist() == [1] * 6 + [0]
    ca, cb = A["camera_to_world"].reshape(4, 4), B["camera_to_world"].reshape(4, 4)
    assert np.array_equal(ca[[0, 1, 3]], cb[[0, 1, 3]]) and np.array_equal(ca[2], -cb[2])
    for k in ("bsdf", "emitter", "radiance", "reflectance", "bsdf_params"):
        assert np.array_equal(A[k], B[k])
    rng = np.random.default_rng(5)
    n = 4099
    o = rng.uniform(-2.5, 2.5, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1)[:, None]).astype(np.float32)
    # the twin test's own rays too: from the camera through the pixel centres
    oc, dc = tf.camera_rays(A)
    o, d = np.concatenate([o, oc]), np.concatenate([d, dc])
    m = np.array([1, 1, -1], np.float32)
    pa, ta = pkg.intersect_host(A, o, d)
    pb, tb = pkg.intersect_host(B, o * m, d * m)
    assert np.array_equal(pa, pb) and np.array_equal(ta.view(np.uint32), tb.view(np.uint32))
    assert (pa[:n] == tf.PROBE).sum() > 100 and (pa[n:] == tf.PROBE).all() and (pa >= 0).all()
    # the mirrored camera produces the mirrored rays
    ob, db = tf.camera_rays(B)
    assert np.array_equal(ob, oc * m) and np.array_equal(db, dc * m)


def test_sheet_scene(pkg, scenes):
    desc = scenes.sheet_scene(48, 27)
    v = desc["mesh_vertices"].reshape(-1, 3)
    tri = desc["triangles"].reshape(-1, 3)
    fn = np.cross(v[tri[:, 1]] - v[tri[:, 0]], v[tri[:, 2]] - v[tri[:, 0]])      # float32, as the library forms it
    assert len(tri) == 2 * 16 * 48 and np.linalg.norm(fn, axis=1).min() > 1e-3
    assert (fn[:, 1] > 0).all()                                 # every face normal on the upper side
    b = int(desc["tri_bsdf"][0])
    assert (desc["tri_bsdf"] == b).all() and desc["bsdf_twosided"][b] == 1 and desc["bsdf_twosided"].sum() == 1
    o, d = tf.camera_rays(desc)
    prim, t = pkg.intersect_host(desc, o, d, 1e-2, np.inf, 0)
    pb, tb = pkg.intersect_host(desc, o, d, 1e-2, np.inf, 1)
    assert np.array_equal(prim, pb) and np.array_equal(t.view(np.uint32), tb.view(np.uint32))
    nq = len(desc["quads"]) // 9
    on = prim >= nq
    back = (d[on].astype(np.float64) * fn[prim[on] - nq]).sum(1) > 0
    frac = float(back.mean())
    print(f"sheet_scene 48 x 27: {int(on.sum())} camera rays on the sheet, {frac:.3f} of them from behind")
    assert on.sum() > 300 and 0.30 <= frac <= 0.70
    # the materials and the one-sided form
    for material, kind in zip(scenes.SHEET_MATERIALS, (0.0, 1.0, 2.0, 3.0, 6.0)):
        dm = scenes.sheet_scene(16, 9, material=material)
        assert dm["bsdf_params"][8 * b] == kind and dm["bsdf_twosided"][b] == 1
    assert "bsdf_twosided" not in scenes.sheet_scene(16, 9, twosided=False)
    env = scenes.sheet_scene(16, 9, environment=scenes.constant_environment((1.0, 1.0, 1.0)))
    assert env["env_kind"] == 1 and len(env["quads"]) == 9      # the floor alone
    with_patch = scenes.sheet_scene(16, 9, patch=True)
    assert with_patch["bsdf_twosided"].tolist() == [0, 0, 1, 0, 1] and with_patch["learned_models"][4] is not None
    pkg.intersect_host(with_patch, o[:4], d[:4])               # validates
