"""Environment emitters on the host (no GPU), through env_eval_host: the
lat-long lookup against numpy restatements, non-finite directions, the constant
emitter, exact rotations and orientation, the description's validation, older
callers' zeroed fields, the unchanged default torus scene and a sanitizer run of
the lookup as a stand-alone program."""
import hashlib
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import env_fixture as ef  # noqa: E402
import mesh_fixture as mf  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("which", range(len(ef.SIZES)))
def test_against_numpy_restatement(pkg, which):
    """Every finite direction within 4x the worst error, on the same map and
    directions, of the numpy float32 restatement against the float64 one (the
    rule tests/test_mesh.py uses for t).  Realised when this was written
    (library / float32 restatement, absolute radiance): 8x4 6.81e-7 / 6.81e-7,
    16x8 9.86e-7 / 9.73e-7, 1x1 2.38e-7 / 2.38e-7, 1x4 4.50e-7 / 4.14e-7, 4x1
    4.72e-7 / 4.72e-7."""
    name, px, scale = ef.maps()[which]
    d, finite = ef.directions()
    M = np.asarray(ef.ROTATIONS["rz90"], np.float32) if which == 1 else None
    got = pkg.env_eval_host(ef.desc_of(px, scale, M), d)
    assert got.shape == (len(d), 3) and got.dtype == np.float32
    r64 = ef.restate(px, scale, M, d[finite], np.float64)
    r32 = ef.restate(px, scale, M, d[finite], np.float32)
    err32 = float(np.abs(r32.astype(np.float64) - r64).max())
    err = float(np.abs(got[finite].astype(np.float64) - r64).max())
    print(f"env {name}: library {err:.3e}, numpy float32 restatement {err32:.3e} (bound 4x = {4 * err32:.3e}), "
          f"{int(finite.sum())} directions")
    assert err32 > 0
    assert err <= 4 * err32
    # the map is seen: the lookups span most of its range (a 1x1 map has one value)
    if px.shape[0] * px.shape[1] > 1:
        assert got[finite].max() > 0.8 * scale * px.max() and got[finite].min() < 1.5 * scale * px.min()


def test_nonfinite_directions_return_zero(pkg):
    d, finite = ef.directions()
    assert (~finite).sum() == 2
    for name, px, scale in ef.maps():
        got = pkg.env_eval_host(ef.desc_of(px, scale), d)
        assert np.all(_bits(got[~finite]) == 0), name
        assert np.all(got[finite] > 0), name


def test_constant_returns_the_radiance_bitwise(pkg, scenes):
    d, finite = ef.directions()
    rad = np.asarray([1.0, 0.8, 0.6], np.float32)
    got = pkg.env_eval_host(scenes.constant_environment(rad), d)
    assert np.all(_bits(got) == _bits(rad)[None, :])
    # no scale, no transform, no map: the other env fields are not read
    noisy = {**scenes.constant_environment(rad), "env_scale": np.nan, "env_world_to_local": np.full(9, np.inf)}
    assert np.all(_bits(pkg.env_eval_host(noisy, d)) == _bits(rad)[None, :])
    assert np.all(_bits(pkg.env_eval_host({"env_kind": 0, "env_radiance": rad}, d)) == 0)


@pytest.mark.parametrize("rot", sorted(ef.ROTATIONS))
def test_signed_permutation_is_exact(pkg, rot):
    """env(M, d) == env(I, M d) bitwise for a signed permutation matrix M."""
    d, finite = ef.directions()
    M = np.asarray(ef.ROTATIONS[rot], np.float32)
    for name, px, scale in ef.maps()[:2]:
        a = pkg.env_eval_host(ef.desc_of(px, scale, M), d)
        b = pkg.env_eval_host(ef.desc_of(px, scale), ef.rotate_exact(M, d))
        assert np.array_equal(_bits(a), _bits(b)), (rot, name)
        c = pkg.env_eval_host(ef.desc_of(px, scale), d)
        assert not np.array_equal(_bits(a), _bits(c)), (rot, name)


def _uv64(v):
    v = np.asarray(v, np.float64)
    return np.mod(np.arctan2(v[:, 0], -v[:, 2]) / (2 * np.pi), 1.0), np.arccos(np.clip(v[:, 1], -1, 1)) / np.pi


@pytest.mark.parametrize("rot", [None, "ry90", "rx90"])
def test_orientation(pkg, rot):
    """A 16x8 map whose only non-zero texels are the 2x2 block of columns 11,
    12 and rows 2, 3: the brightest lookup points into that block, and the
    direction computed here from the block's (u, v) -- inverting u = atan2(x,
    -z) / 2 pi, v = acos(y) / pi -- sees the block's value."""
    px = np.zeros((8, 16, 3), np.float32)
    px[2:4, 11:13] = [3.0, 2.0, 1.0]
    u, v = 12.0 / 16.0, 3.0 / 8.0                       # the block's centre
    theta, phi = np.pi * v, 2 * np.pi * u
    local = np.asarray([np.sin(theta) * np.sin(phi), np.cos(theta), -np.sin(theta) * np.cos(phi)])
    M = np.eye(3) if rot is None else np.asarray(ef.ROTATIONS[rot], np.float64)
    target = M.T @ local                                # world direction: M target = local
    d, finite = ef.directions()
    dirs = np.concatenate([d[finite], target[None].astype(np.float32)])
    got = pkg.env_eval_host(ef.desc_of(px, 1.0, M), dirs)
    assert np.abs(got[-1] - np.asarray([3.0, 2.0, 1.0])).max() < 1e-5
    best = int(np.argmax(got.sum(-1)))
    bu, bv = _uv64(dirs[best:best + 1].astype(np.float64) @ M.T)
    assert 11.0 / 16 <= bu[0] <= 13.0 / 16 and 2.0 / 8 <= bv[0] <= 4.0 / 8, (best, bu, bv)
    # everything away from the block (a texel further out) is black
    au, av = _uv64(dirs.astype(np.float64) @ M.T)
    far = (au < 10.0 / 16) | (au > 14.0 / 16) | (av < 1.0 / 8) | (av > 5.0 / 8)
    assert far.sum() > 3000 and np.all(got[far] == 0)
    lit = (au > 11.6 / 16) & (au < 12.4 / 16) & (av > 2.6 / 8) & (av < 3.4 / 8)
    assert lit.sum() >= 1 and np.abs(got[lit, 0] - 3.0).max() < 1e-5


def _expect_invalid(pkg, desc, word):
    with pytest.raises(pkg.SDMMError, match="sdmm error -1") as e:
        pkg.env_eval_host(desc, np.asarray([[0.0, 1.0, 0.0]], np.float32))
    assert word in str(e.value), str(e.value)
    assert word in pkg.lib().sdmm_last_error().decode()


def test_validation(pkg, scenes):
    px = ef.maps()[0][1]
    good = ef.desc_of(px, 1.0, np.eye(3))
    pkg.env_eval_host(good, np.zeros((1, 3), np.float32))
    _expect_invalid(pkg, {**good, "env_kind": 3}, "env_kind")
    _expect_invalid(pkg, {**good, "env_kind": -1}, "env_kind")
    _expect_invalid(pkg, {"env_kind": 2}, "env_pixels")
    for bad in (np.nan, np.inf, -0.5):
        p = px.copy()
        p[3, 7, 2] = bad
        _expect_invalid(pkg, {**good, "env_pixels": p}, "texel")
        _expect_invalid(pkg, {**good, "env_scale": bad}, "env_scale")
        _expect_invalid(pkg, {"env_kind": 1, "env_radiance": [1.0, bad, 1.0]}, "env_radiance")
    for bad in (np.nan, -np.inf):
        m = np.eye(3, dtype=np.float32)
        m[1, 2] = bad
        _expect_invalid(pkg, {**good, "env_world_to_local": m}, "env_world_to_local")
    # sizes the binding cannot express from an array's shape: through the struct
    sd, keep = pkg._SceneDesc(), {}
    pkg._fill_env(sd, good, keep)
    dd, out = np.asarray([[0.0, 1.0, 0.0]], np.float32), np.zeros((1, 3), np.float32)

    def call():
        return pkg.lib().sdmm_env_eval_host(pkg.C.byref(sd), 1, dd.ctypes.data, out.ctypes.data)
    assert call() == 0
    for w, h, word in ((0, 4, "< 1"), (8, 0, "< 1"), (-8, 4, "< 1"), (1 << 14, (1 << 12) + 1, "2^26")):
        sd.env_width, sd.env_height = w, h
        assert call() == -1
        assert word in pkg.lib().sdmm_last_error().decode()
    sd.env_width, sd.env_height, sd.env_pixels = 8, 4, None
    assert call() == -1 and "env_pixels" in pkg.lib().sdmm_last_error().decode()


def test_zeroed_trailing_fields(pkg, scenes):
    """An older caller's description -- every env field zero, the scale and the
    matrix included -- validates, intersects as before and has no environment."""
    o, d, _ = mf.rays(scenes)
    desc = mf.torus_desc(scenes)
    ref = pkg.intersect_host(desc, o, d, mf.MINT, np.inf, 0)
    sd, keep = pkg._SceneDesc(), {}
    pkg._fill_geometry(sd, desc, keep)
    sd.env_kind, sd.env_width, sd.env_height, sd.env_pixels, sd.env_scale = 0, 0, 0, None, 0.0
    for i in range(9):
        sd.env_world_to_local[i] = 0.0
    for i in range(3):
        sd.env_radiance[i] = 0.0
    prim, t = np.empty(len(o), np.int32), np.empty(len(o), np.float32)
    pkg._check(pkg.lib().sdmm_scene_intersect_host(pkg.C.byref(sd), len(o), o.ctypes.data, d.ctypes.data, mf.MINT,
                                                   float("inf"), 0, prim.ctypes.data, t.ctypes.data))
    assert np.array_equal(prim, ref[0]) and np.array_equal(_bits(t), _bits(ref[1]))
    rgb = np.ones((len(d), 3), np.float32)
    pkg._check(pkg.lib().sdmm_env_eval_host(pkg.C.byref(sd), len(d), d.ctypes.data, rgb.ctypes.data))
    assert np.all(_bits(rgb) == 0)


# torus_scene() as the commit before the environment emitter built it: SHA-256
# of every array's bytes (dtype, shape), computed once from that commit
_TORUS_DEFAULT = {
    "bsdf": ("int32", (13,), "bafbe8e3ba630ea00bd888505f83da3dbc49b8afc84056a64447f8971fad5e34"),
    "bsdf_params": ("float32", (40,), "87367dae643a9ce775b12fb72f863ff091c91155d809771630ef0efc50723d35"),
    "camera_to_world": ("float32", (16,), "ecafcfcc2c4ca2461cb16080d29deee23e42aeb4eb43a8406297a6c313c995bb"),
    "emitter": ("int32", (13,), "5dc63f3b9eb67260d0b84cab8df636a19b1e6ab2bdf1c9aadc0c6fd9b6bdcd91"),
    "mesh_vertices": ("float32", (13824,), "bfbdcbb9188f69c013005b358bc2071fe91461e2324fcf3876aa6f88e7876fb4"),
    "quads": ("float32", (117,), "4ce4b0ebebe4074daa86dde7a66e4bcdc3168ca9150231932c2ba10a74c16a3a"),
    "radiance": ("float32", (3,), "2875dc753eb29e81ff832dbe485d37e55cdcee21753cceb44bc35f74b329198c"),
    "reflectance": ("float32", (15,), "337bfaea618fee0bc94ddfa31bb4def3d6d5ff34154d07d98e38f6d0a9fad640"),
    "tri_bsdf": ("int32", (9216,), "d5a249ace52d0ca2297244dd640c6c47da1a79254af28ea26f97e00be42535b4"),
    "triangles": ("int32", (27648,), "3cad5577c8d031881a5b119a84f3597962d0c2aa3ca817175ab46efeb6f58a0c"),
}
_TORUS_DEFAULT_SCALARS = {"fov_x_deg": 45.0, "height": 360, "near_clip": 0.01, "width": 640}
_TORUS_DEFAULT_MODEL = "8a2b97d42315a9ed043e83d3522d3f04c95b46c78f50947e9c366362607cff22"


def test_default_torus_scene_is_unchanged(pkg, scenes):
    """torus_scene() (environment=None) builds the closed room of before, array
    for array; with an environment the room and the lamp are gone."""
    d = scenes.torus_scene()
    arrays = {k: v for k, v in d.items() if isinstance(v, np.ndarray)}
    assert sorted(arrays) == sorted(_TORUS_DEFAULT)
    for k, (dtype, shape, sha) in _TORUS_DEFAULT.items():
        a = arrays[k]
        assert str(a.dtype) == dtype and a.shape == shape, k
        assert hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest() == sha, k
    assert {k: v for k, v in d.items() if not isinstance(v, (np.ndarray, list))} == _TORUS_DEFAULT_SCALARS
    models = d["learned_models_nd"]
    assert [m is None for m in models] == [True, True, True, False, True]
    assert hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in models[3])).hexdigest() == \
        _TORUS_DEFAULT_MODEL
    assert sorted(k for k, v in d.items() if isinstance(v, list)) == ["learned_models_nd"]
    # the open scene: the floor and the case only, no emitter quad, the same mesh and camera
    sky = scenes.sky_environment(64, 32)
    e = scenes.torus_scene(environment=sky)
    assert e["quads"].size // 9 == 1 + 6 and np.all(e["emitter"] == -1)
    assert e["env_kind"] == 2 and e["env_pixels"].shape == (32, 64, 3)
    for k in ("mesh_vertices", "triangles", "tri_bsdf", "camera_to_world", "reflectance", "bsdf_params"):
        assert np.array_equal(e[k], d[k]), k
    q = d["quads"].reshape(13, 9)                        # room 5, floor, lamp, case 6
    assert np.array_equal(e["quads"].reshape(7, 9), np.concatenate([q[5:6], q[7:13]]))
    # the sky: a sun far brighter than the gradient, in the upper half
    px = sky["env_pixels"].astype(np.float64)
    assert np.isfinite(px).all() and px.min() > 0
    row = np.unravel_index(np.argmax(px.sum(-1)), px.shape[:2])[0]
    assert row < 16 and px.max() > 50 * np.median(px)
    c = scenes.constant_environment((1, 0.8, 0.6))
    assert c["env_kind"] == 1 and c["env_radiance"].dtype == np.float32


def test_sanitizer_standalone(pkg, scenes, tmp_path):
    """tests/cpp/env_check.cpp with envmap.h under ASan + UBSan as a program of
    its own (nothing is preloaded): every map of the fixture (identity and a
    rotation), a constant emitter and the orientation map against every
    direction; its outputs are the library's bitwise."""
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
    d, _ = ef.directions()
    cases = []                                           # (description, kind, pixels, scale, rad, M)
    for name, px, scale in ef.maps():
        for M in (np.eye(3, dtype=np.float32), np.asarray(ef.ROTATIONS["cyc"], np.float32)):
            cases.append((ef.desc_of(px, scale, M), 2, px, scale, np.zeros(3, np.float32), M))
    rad = np.asarray([1.0, 0.8, 0.6], np.float32)
    cases.append((scenes.constant_environment(rad), 1, None, 0.0, rad, np.zeros((3, 3), np.float32)))
    fx = tmp_path / "fixture.bin"
    with open(fx, "wb") as f:
        np.asarray([len(cases), len(d)], np.int32).tofile(f)
        d.tofile(f)
        for _, kind, px, scale, r3, M in cases:
            h, w = (0, 0) if px is None else px.shape[:2]
            np.asarray([kind, w, h], np.int32).tofile(f)
            np.concatenate([[scale], r3, np.asarray(M, np.float32).reshape(-1)]).astype(np.float32).tofile(f)
            if px is not None:
                np.ascontiguousarray(px, np.float32).tofile(f)
    csrc = ROOT / "sdmm-mitsuba_amd" / "csrc"
    exe = tmp_path / "env_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", *flags, f"-I{csrc}",
                    str(ROOT / "tests" / "cpp" / "env_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), str(fx)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0
    assert "env_check ok" in r.stdout
    got = np.fromfile(tmp_path / "fixture.bin.out", np.float32).reshape(len(cases), len(d), 3)
    for i, (desc, *_rest) in enumerate(cases):
        assert np.array_equal(_bits(got[i]), _bits(pkg.env_eval_host(desc, d))), i
