"""Host: bitmap textures on reflectances (sdmm_scene_desc.mesh_uvs, textures,
bsdf_texture) -- sdmm_scene_texture_host against the numpy float32 restatement
of csrc/texture.h (tests/texture_cases.py), the validation messages and their
place after every older check, mirror_z with textures, the scene helpers, and
csrc/texture.h under ASan + UBSan as a program of its own.  No GPU."""
import copy
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import texture_cases as tc

ROOT = Path(__file__).resolve().parents[1]
F = np.float32
NAN, INF = F(np.nan), F(np.inf)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want, what):
    bad = np.nonzero((_bits(got) != _bits(want)).reshape(len(got), -1).any(1))[0]
    assert not len(bad), (what, len(bad), bad[:5], got[bad[:3]], want[bad[:3]])


# ---- 1: the host entry is the restatement, bitwise ----------------------------------------
@pytest.mark.parametrize("geometry", tc.GEOMETRIES)
def test_texture_host_equals_restatement(pkg, geometry):
    desc, o, d = tc.sweep(geometry)
    prim, t, uv, rgb = pkg.texture_host(desc, o, d)
    p0, t0 = pkg.intersect_host(desc, o, d)
    assert np.array_equal(prim, p0) and np.array_equal(_bits(t), _bits(t0))
    assert (prim >= 0).all() and (t == 1.0).all()
    want_uv, want_rgb = tc.restate(desc, o, d, prim)
    _same(uv, want_uv, geometry + " uv")
    _same(rgb, want_rgb, geometry + " rgb")
    # the BVH and the loop over all triangles agree
    prim1, t1, uv1, rgb1 = pkg.texture_host(desc, o, d, mode=1)
    assert np.array_equal(prim, prim1)
    _same(uv1, uv, "mode 1 uv")
    _same(rgb1, rgb, "mode 1 rgb")


def test_probe_uvs_equal_restatement(pkg):
    desc, o, d = tc.probe()
    prim, t, uv, rgb = pkg.texture_host(desc, o, d)
    assert (prim >= 0).all()
    want_uv, want_rgb = tc.restate(desc, o, d, prim)
    _same(uv, want_uv, "probe uv")
    _same(rgb, want_rgb, "probe rgb")
    # through the vertex the uv is the entry itself (every second ray)
    m = len(tc.PROBE_UVS)
    through = uv[0::2].reshape(-1, m, 2)
    assert (through == tc.PROBE_UVS[None]).all()
    # a texel coordinate past int32, and a scaled uv that overflows: 0, whatever the wrap
    texs = desc["textures"]
    per = rgb[0::2].reshape(len(texs), m, 3)
    for i, tex in enumerate(texs):
        if tex["uv_scale"][0] == 7.5:
            assert (per[i, 2] == 0).all() and (per[i, 3] == 0).all(), i        # 3e38 * 7.5 = inf
        assert (per[i, 0] == 0).all() and (per[i, 1] == 0).all(), i            # 1e9 * 3, * 5 leave int32


def test_cases_reach_what_they_are_for(pkg):
    """The sweep's uvs hold the families named in its docstrings, and the
    restatement's own pieces behave as the reference states them."""
    desc, o, d = tc.sweep("quad", tc.configs()[:1])
    _, _, uv, _ = pkg.texture_host(desc, o, d)
    assert (uv == 0).any() and (uv == 1).any() and np.isin(uv, np.arange(9) / 8.0).all(1).sum() == 81
    desc, o, d = tc.sweep("mesh_uv", tc.configs()[:1])
    _, _, uv, _ = pkg.texture_host(desc, o, d)
    assert (uv < 0).any() and (uv > 1).any()
    assert np.array_equal(uv[0], tc.SQUARE_UVS[0]) and np.array_equal(uv[80], tc.SQUARE_UVS[2])   # corners
    desc, o, d = tc.sweep("mesh_bary", tc.configs()[:1])
    prim, _, uv, _ = pkg.texture_host(desc, o, d)
    assert set(prim) == {0, 1} and (uv >= 0).all() and (uv.sum(1) <= 1).all()
    # evalTexel's rules by hand on a row of three texels 10, 20, 30
    tex = {"pixels": np.asarray([[[10] * 3, [20] * 3, [30] * 3]], F), "filter": 1, "wrap_v": 1}
    x = np.asarray([-4, -3, -2, -1, 0, 1, 2, 3, 4, 5, 6], F)
    uvs = np.stack([(x + F(0.5)) / F(3), np.full(len(x), 0.5, F)], -1)
    want = {0: [30, 10, 20, 30, 10, 20, 30, 10, 20, 30, 10], 1: [10, 10, 10, 10, 10, 20, 30, 30, 30, 30, 30],
            2: [30, 30, 20, 10, 10, 20, 30, 30, 20, 10, 10], 3: [0, 0, 0, 0, 10, 20, 30, 0, 0, 0, 0],
            4: [1, 1, 1, 1, 10, 20, 30, 1, 1, 1, 1]}
    for wu, row in want.items():
        assert list(tc.tex_eval({**tex, "wrap_u": wu}, uvs)[:, 0]) == row, wu
    # bilinear at a texel centre is that texel, half-way the mean (exact: dyadic weights)
    bil = {**tex, "filter": 0, "wrap_u": 1}
    got = tc.tex_eval(bil, np.asarray([[0.5, 0.5], [2.0 / 3.0, 0.5]], F))[:, 0]
    assert got[0] == 20 and abs(got[1] - 25) < 1e-4


def test_untextured_bsdf_reports_its_row_and_the_uv(pkg):
    desc, o, d = tc.sweep("quad", tc.configs()[:2])
    desc["bsdf_texture"] = np.asarray([-1, 1], np.int32)
    prim, _, uv, rgb = pkg.texture_host(desc, o, d)
    first = prim == 0
    assert first.sum() == len(tc.cell_points())
    assert (rgb[first] == desc["reflectance"][:3]).all()
    want_uv, want_rgb = tc.restate(desc, o, d, prim)
    _same(uv, want_uv, "uv")
    _same(rgb, want_rgb, "rgb")
    assert (uv[first] == tc.cell_points()).all()
    # no texture fields at all: the row and the uv still
    bare = {k: v for k, v in desc.items() if k not in ("textures", "bsdf_texture")}
    _, _, uv_b, rgb_b = pkg.texture_host(bare, o, d)
    _same(uv_b, uv, "bare uv")
    assert (rgb_b == desc["reflectance"][:3]).all()
    # a miss: zeros
    p, _, uv_m, rgb_m = pkg.texture_host(desc, [[0.5, 1.0, 0.5]], [[0.0, 1.0, 0.0]])
    assert p[0] == -1 and (uv_m == 0).all() and (rgb_m == 0).all()


# ---- 2: validation ----------------------------------------------------------------------
def _tex(**kw):
    return {"pixels": tc.pixels(2, 2), **kw}


def _outcome(pkg, call):
    try:
        call()
    except pkg.SDMMError as e:
        return None if str(e).startswith("sdmm error -2: ") else str(e)
    return None


HOST, CREATE = "sdmm_scene_texture_host", "sdmm_scene_create"


def _table():
    """(label, changes to the textured description, message or None)."""
    rows = [
        ("plain", {}, None),
        ("no textures, no bsdf_texture", {"textures": None, "bsdf_texture": None}, None),
        ("textures unused", {"bsdf_texture": None}, None),
        ("index -1", {"bsdf_texture": [-1, -1]}, None),
        ("index n - 1", {"bsdf_texture": [1, 0]}, None),
        ("index n", {"bsdf_texture": [2, 0]}, "a bsdf_texture entry outside -1 .. n_textures - 1"),
        ("index -2", {"bsdf_texture": [-2, 0]}, "a bsdf_texture entry outside -1 .. n_textures - 1"),
        ("bsdf_texture alone", {"textures": None}, "bsdf_texture without textures"),
        ("filter 1", {"textures": [_tex(filter=1), _tex()]}, None),
        ("filter 2", {"textures": [_tex(filter=2), _tex()]}, "a texture's filter outside 0..1"),
        ("filter -1", {"textures": [_tex(filter=-1), _tex()]}, "a texture's filter outside 0..1"),
        ("wrap 4", {"textures": [_tex(wrap_u=4, wrap_v=4), _tex()]}, None),
        ("wrap_u 5", {"textures": [_tex(wrap_u=5), _tex()]}, "a texture's wrap_u or wrap_v outside 0..4"),
        ("wrap_v 5", {"textures": [_tex(), _tex(wrap_v=5)]}, "a texture's wrap_u or wrap_v outside 0..4"),
        ("wrap_u -1", {"textures": [_tex(wrap_u=-1), _tex()]}, "a texture's wrap_u or wrap_v outside 0..4"),
        ("scale 0", {"textures": [_tex(uv_scale=(0.0, 1.0)), _tex()]}, "a texture's uv_scale is 0 or not finite"),
        ("scale -0", {"textures": [_tex(uv_scale=(1.0, -0.0)), _tex()]}, "a texture's uv_scale is 0 or not finite"),
        ("scale nan", {"textures": [_tex(uv_scale=(NAN, 1.0)), _tex()]}, "a texture's uv_scale is 0 or not finite"),
        ("scale inf", {"textures": [_tex(uv_scale=(1.0, INF)), _tex()]}, "a texture's uv_scale is 0 or not finite"),
        ("scale tiny", {"textures": [_tex(uv_scale=(F(2.0 ** -126), -3e38)), _tex()]}, None),
        ("offset inf", {"textures": [_tex(uv_offset=(0.0, -INF)), _tex()]}, "a texture's uv_offset is not finite"),
        ("offset big", {"textures": [_tex(uv_offset=(3e38, -3e38)), _tex()]}, None),
        ("texel 0", {"textures": [_tex(pixels=np.zeros((1, 1, 3), F)), _tex()]}, None),
        ("texel negative", {"textures": [_tex(pixels=np.asarray([[[0.5, -1e-30, 0.5]]], F)), _tex()]},
         "a non-finite or negative texel"),
        ("texel nan", {"textures": [_tex(), _tex(pixels=np.asarray([[[0.5, 0.5, NAN]]], F))]},
         "a non-finite or negative texel"),
    ]
    return rows


@pytest.fixture(scope="module")
def two(pkg):
    """Two unit squares (quads) with a texture each."""
    desc, o, d = tc.sweep("quad", [_tex(), _tex(filter=1)])
    return tc.camera_fields(desc), o, d


def _changed(desc, changes):
    c = {k: v for k, v in desc.items()}
    for k, v in changes.items():
        if v is None:
            c.pop(k, None)
        else:
            c[k] = np.asarray(v, np.int32) if k == "bsdf_texture" else v
    return c


def test_validation_messages(pkg, two):
    desc, o, d = two
    wrong = []
    for label, changes, msg in _table():
        c = _changed(desc, changes)
        for who, call in ((HOST, lambda: pkg.texture_host(c, o[:1], d[:1])), (CREATE, lambda: pkg.Scene(c))):
            want = None if msg is None else f"sdmm error -1: {who}: {msg}"
            got = _outcome(pkg, call)
            if got != want:
                wrong.append(f"{label} [{who}]: got {got!r}, want {want!r}")
    assert not wrong, "\n".join(wrong)


def test_texel_cap(pkg, two):
    """2^26 texels in all are accepted (the host entry reads them in place: an
    untouched block of zeros), one texture more is not -- the cap is tested
    before any texel is read."""
    desc, o, d = two
    wide = np.zeros((8192, 8192, 3), F)
    c = _changed(desc, {"textures": [{"pixels": wide}], "bsdf_texture": [0, -1]})
    assert _outcome(pkg, lambda: pkg.texture_host(c, o[:1], d[:1])) is None
    c = _changed(desc, {"textures": [{"pixels": wide}, _tex()], "bsdf_texture": [0, -1]})
    for who, call in ((HOST, lambda: pkg.texture_host(c, o[:1], d[:1])), (CREATE, lambda: pkg.Scene(c))):
        assert _outcome(pkg, call) == f"sdmm error -1: {who}: textures of more than 2^26 texels in all"


def _raw_desc(pkg, desc):
    sd, keep = pkg._SceneDesc(), {}
    pkg._fill_geometry(sd, desc, keep)
    return sd, keep


def test_validation_of_raw_fields(pkg, two):
    """What the Python wrapper cannot express: a zeroed sdmm_texture, a null
    pixels pointer, a width or height below 1, a negative n_textures, textures
    NULL with a count."""
    import ctypes as C
    desc, o, d = two
    o1, d1 = np.ascontiguousarray(o[:1]), np.ascontiguousarray(d[:1])
    out = [np.empty(1, np.int32), np.empty(1, F), np.empty((1, 2), F), np.empty((1, 3), F)]

    def run(mutate):
        sd, keep = _raw_desc(pkg, desc)
        tab = keep["textures"]
        mutate(sd, tab)
        rc = pkg.lib().sdmm_scene_texture_host(C.byref(sd), 1, o1.ctypes.data, d1.ctypes.data, 1e-4, float("inf"), 0,
                                               *[a.ctypes.data for a in out])
        return rc, pkg.lib().sdmm_last_error().decode() if rc else ""

    def zeroed(sd, tab):
        px, w, h = tab[0].pixels, tab[0].width, tab[0].height
        C.memset(C.byref(tab[0]), 0, C.sizeof(tab[0]))
        tab[0].pixels, tab[0].width, tab[0].height = px, w, h
    assert run(lambda sd, tab: None) == (0, "")
    assert run(zeroed) == (-1, f"{HOST}: a texture's uv_scale is 0 or not finite")
    assert run(lambda sd, tab: setattr(tab[1], "pixels", None)) == (-1, f"{HOST}: a texture without pixels")
    assert run(lambda sd, tab: setattr(tab[0], "width", 0)) == (-1, f"{HOST}: a texture's width or height < 1")
    assert run(lambda sd, tab: setattr(tab[1], "height", -3)) == (-1, f"{HOST}: a texture's width or height < 1")
    assert run(lambda sd, tab: setattr(tab[1], "height", 1)) == (0, "")
    both = f"{HOST}: n_textures < 0, or textures NULL with n_textures > 0"
    assert run(lambda sd, tab: setattr(sd, "n_textures", -1)) == (-1, both)
    assert run(lambda sd, tab: setattr(sd, "textures", None)) == (-1, both)
    # the order inside one texture: size, pixels, the cap, filter, wrap, scale, offset, texels
    def two_wrong(a, b):
        def m(sd, tab):
            a(tab[0])
            b(tab[0])
        return m
    size = lambda t: setattr(t, "width", 0)
    nopx = lambda t: setattr(t, "pixels", None)
    filt = lambda t: setattr(t, "filter", 7)
    wrap = lambda t: setattr(t, "wrap_v", 7)
    scale = lambda t: t.uv_scale.__setitem__(0, 0.0)
    offs = lambda t: t.uv_offset.__setitem__(1, float("inf"))
    msgs = [(size, "a texture's width or height < 1"), (nopx, "a texture without pixels"),
            (filt, "a texture's filter outside 0..1"), (wrap, "a texture's wrap_u or wrap_v outside 0..4"),
            (scale, "a texture's uv_scale is 0 or not finite"), (offs, "a texture's uv_offset is not finite")]
    for i in range(len(msgs)):
        for j in range(i + 1, len(msgs)):
            assert run(two_wrong(msgs[j][0], msgs[i][0])) == (-1, f"{HOST}: {msgs[i][1]}"), (i, j)


def test_kinds_that_take_a_texture(pkg, scenes):
    """bsdf_texture on kinds 0, 1 and 3 only; and after every older check."""
    names = list(scenes._BSDFS)
    kinds = {1: "Floor", 2: "TallBox", 3: "ShortBox", 4: "LeftWall", 5: "RightWall", 6: "BackWall"}
    box = scenes.cornell_box(32, 18, plastic=(kinds[1],), conductor=(kinds[2],), phong=(kinds[3],),
                             dielectric=(kinds[4],), glass=(kinds[5],), mirror=(kinds[6],))
    box["textures"] = [_tex()]
    msg = "bsdf_texture on a BSDF of kind 2, 4, 5 or 6 (only the reflectance of kinds 0, 1 and 3 takes a texture)"
    for kind, name in {0: "Ceiling", **kinds}.items():
        bt = np.full(len(names), -1, np.int32)
        bt[names.index(name)] = 0
        c = {**box, "bsdf_texture": bt}
        want = None if kind in (0, 1, 3) else f"sdmm error -1: {CREATE}: {msg}"
        assert _outcome(pkg, lambda: pkg.Scene(c)) == want, kind
        want = None if kind in (0, 1, 3) else f"sdmm error -1: {HOST}: {msg}"
        assert _outcome(pkg, lambda: pkg.texture_host(c, [[0, 1, 0]], [[0, 0, -1]])) == want, kind
    # the new checks come last: each older rejection wins over a texture fault
    bad_tex = {"textures": [_tex(filter=9)], "bsdf_texture": np.full(len(names), -1, np.int32)}
    older = [
        ({"bsdf_params": np.where(np.arange(box["bsdf_params"].size) == 8 * names.index(kinds[2]) + 6, F(0),
                                  box["bsdf_params"]).astype(F)}, "invalid bsdf_params"),
        ({"bsdf_twosided": np.full(len(names), 2, np.int32)}, "a bsdf_twosided entry other than 0 or 1"),
        ({"env_kind": 3}, "env_kind outside 0..2"),
        ({"bsdf": np.full(box["bsdf"].size, 99, np.int32)}, "material index out of range"),
    ]
    for changes, m in older:
        c = {**box, **bad_tex, **changes}
        assert _outcome(pkg, lambda: pkg.Scene(c)) == f"sdmm error -1: {CREATE}: {m}", m
    assert _outcome(pkg, lambda: pkg.Scene({**box, **bad_tex})) == \
        f"sdmm error -1: {CREATE}: a texture's filter outside 0..1"


def test_mesh_uvs_validation(pkg, two):
    desc, o, d = tc.sweep("mesh_uv", [_tex()])
    desc = tc.camera_fields(desc)
    for who, call in ((HOST, lambda c: pkg.texture_host(c, o[:1], d[:1])), (CREATE, lambda c: pkg.Scene(c))):
        assert _outcome(pkg, lambda: call(desc)) is None
        bad = copy.deepcopy(desc)
        bad["mesh_uvs"][3] = INF
        assert _outcome(pkg, lambda: call(bad)) == f"sdmm error -1: {who}: a non-finite mesh_uvs value"
        big = copy.deepcopy(desc)
        big["mesh_uvs"][3] = -3e38
        assert _outcome(pkg, lambda: call(big)) is None
    # mesh_uvs on a scene of quads only: the raw field (the wrapper counts vertices)
    import ctypes as C
    qdesc, qo, qd = two
    sd, keep = _raw_desc(pkg, qdesc)
    uvs = np.zeros(8, F)
    sd.mesh_uvs = uvs.ctypes.data
    out = [np.empty(1, np.int32), np.empty(1, F), np.empty((1, 2), F), np.empty((1, 3), F)]
    o1, d1 = np.ascontiguousarray(qo[:1]), np.ascontiguousarray(qd[:1])
    rc = pkg.lib().sdmm_scene_texture_host(C.byref(sd), 1, o1.ctypes.data, d1.ctypes.data, 1e-4, float("inf"), 0,
                                           *[a.ctypes.data for a in out])
    assert rc == -1 and pkg.lib().sdmm_last_error().decode() == f"{HOST}: mesh_uvs without triangles"
    with pytest.raises(pkg.SDMMError, match="mesh_uvs: 2 floats per mesh vertex"):
        pkg.texture_host({**desc, "mesh_uvs": np.zeros(6, F)}, o[:1], d[:1])


# ---- 3: mirror_z ------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", tc.GEOMETRIES)
def test_mirror_z_with_textures_is_exact(pkg, scenes, geometry):
    desc, o, d = tc.sweep(geometry, tc.configs()[::37])
    desc = tc.camera_fields(desc)
    twin = scenes.mirror_z(desc)
    for k in ("textures", "bsdf_texture", "mesh_uvs"):
        if k in desc:
            assert twin[k] is desc[k] or np.array_equal(twin[k], desc[k]), k
    back = scenes.mirror_z(twin)
    for k, v in desc.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(back[k], v), k
    om, dm = o * np.asarray([1, 1, -1], F), d * np.asarray([1, 1, -1], F)
    prim, t, uv, rgb = pkg.texture_host(desc, o, d)
    prim_m, t_m, uv_m, rgb_m = pkg.texture_host(twin, om, dm)
    assert np.array_equal(prim, prim_m) and np.array_equal(_bits(t), _bits(t_m))
    # (a barycentric that is a sum of signed zeros may come out as the other zero: equal, not the same bits)
    assert np.array_equal(uv_m, uv)
    _same(uv_m + F(0.0), uv + F(0.0), "mirrored uv")
    _same(rgb_m, rgb, "mirrored rgb")


# ---- the scene helpers ------------------------------------------------------------------
def test_scene_helpers(pkg, scenes):
    ck = scenes.checker_texture(4, 3, (0.8, 0.7, 0.6), (0.1, 0.2, 0.3))
    px = ck["pixels"]
    assert px.shape == (3, 4, 3) and px.dtype == np.float32
    assert (px[0, 0] == F([0.8, 0.7, 0.6])).all() and (px[0, 1] == F([0.1, 0.2, 0.3])).all() and (px[1, 1] == px[0, 0]).all()
    rp = scenes.ramp_texture(3, 5)
    assert rp["pixels"].shape == (5, 3, 3) and (np.diff(rp["pixels"][:, :, 0], axis=1) > 0).all()
    assert (np.diff(rp["pixels"][:, :, 1], axis=0) > 0).all()
    assert np.allclose(scenes.texture_mean(ck), 0.5 * (px[0, 0] + px[0, 1]))
    # the sampling weight from the texture's mean
    bp, d = scenes.phong_params(scenes.texture_mean(rp), (0.4, 0.4, 0.4), 30.0)
    assert bp[0] == 3 and 0 < bp[5] < 1
    box = scenes.cornell_box(32, 18, textured=True)
    names = list(scenes._BSDFS)
    bt = box["bsdf_texture"]
    assert bt[names.index("Floor")] == 0 and bt[names.index("BackWall")] == 1 and (np.delete(bt, [names.index("Floor"), names.index("BackWall")]) == -1).all()
    assert box["bsdf_params"].reshape(-1, 8)[names.index("BackWall"), 0] == 3
    assert _outcome(pkg, lambda: pkg.Scene(box)) is None
    with pytest.raises(ValueError):
        scenes.cornell_box(32, 18, textured=True, plastic=("Floor",))
    plain = scenes.cornell_box(32, 18)
    assert "textures" not in plain and "bsdf_texture" not in plain
    # the floor's checker is seen from the camera: both colours among the hits on it
    W, H = 32, 18
    cam = np.asarray(box["camera_to_world"], np.float64).reshape(4, 4)
    o = np.tile(cam[:3, 3], (W * H, 1))
    ys, xs = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    tan = np.tan(np.radians(35.0) / 2)
    l = np.stack([(1 - 2 * xs / W) * tan, (1 - 2 * ys / H) * tan * H / W, np.ones_like(xs)], -1).reshape(-1, 3)
    dd = l @ cam[:3, :3].T
    prim, _, uv, rgb = pkg.texture_host(box, o, dd)
    floor = np.nonzero(box["bsdf"] == names.index("Floor"))[0]
    on = np.isin(prim, floor)
    assert on.sum() > 20 and len(np.unique(_bits(rgb[on])[:, 0])) == 2
    wall = np.isin(prim, np.nonzero(box["bsdf"] == names.index("BackWall"))[0])
    assert wall.sum() > 50 and len(np.unique(_bits(rgb[wall])[:, 0])) > 20
    # meshes that carry uvs
    v, t, n, uvs = scenes.sheet_mesh(4, 6, normals=True, uvs=True)
    assert uvs.shape == (len(v), 2) and uvs.min() == 0 and uvs.max() == 1
    v, t, uvs = scenes.torus_mesh(8, 4, uvs=True)
    assert uvs.shape == (len(v), 2) and uvs.min() == 0 and uvs.max() < 1
    sheet = scenes.sheet_scene(32, 18, nx=4, nz=8, texture=scenes.checker_texture(4, 4), environment=scenes.constant_environment((1, 1, 1)))
    assert sheet["mesh_uvs"].size == 2 * sheet["mesh_vertices"].size // 3 and sheet["bsdf_texture"].tolist() == [-1, -1, 0, -1]
    assert _outcome(pkg, lambda: pkg.Scene(sheet)) is None
    with pytest.raises(ValueError):
        scenes.sheet_scene(32, 18, material="mirror", texture=scenes.checker_texture(4, 4))
    # a filter or wrap name the wrapper does not know: its own error, as for a wrong shape
    for key, value in (("filter", "cubic"), ("wrap_u", "wrap"), ("wrap_v", "black")):
        bad = {**sheet, "textures": [scenes.checker_texture(4, 4, **{key: value})]}
        with pytest.raises(pkg.SDMMError, match=f"a texture's {key}"):
            pkg.Scene(bad)


# ---- 4: csrc/texture.h under the sanitizers, a program of its own -----------------------
def test_sanitizer_standalone(pkg, tmp_path):
    """tests/cpp/texture_check.cpp with texture.h under ASan + UBSan as a
    program of its own (nothing is preloaded): every texture of the sweep
    against edge_uvs() through tex_eval, read in place and as RGBA texels, and
    the uv helpers; its outputs are the restatement's bitwise."""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler on this machine")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
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
    uvs = tc.edge_uvs()
    texs = tc.configs()
    fx = tmp_path / "fixture.bin"
    with open(fx, "wb") as f:
        np.asarray([len(texs), len(uvs)], np.int32).tofile(f)
        uvs.tofile(f)
        for t in texs:
            h, w = t["pixels"].shape[:2]
            np.asarray([w, h, t["filter"], t["wrap_u"], t["wrap_v"]], np.int32).tofile(f)
            np.asarray([*t["uv_scale"], *t["uv_offset"]], F).tofile(f)
            np.ascontiguousarray(t["pixels"], F).tofile(f)
    csrc = ROOT / "sdmm-mitsuba_amd" / "csrc"
    exe = tmp_path / "texture_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", *flags, f"-I{csrc}",
                    str(ROOT / "tests" / "cpp" / "texture_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), str(fx)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0
    assert "texture_check ok" in r.stdout
    got = np.fromfile(tmp_path / "fixture.bin.out", F).reshape(len(texs), len(uvs), 3)
    for i, t in enumerate(texs):
        want = tc.tex_eval(t, uvs)
        assert np.array_equal(_bits(got[i]), _bits(want)), (i, {k: v for k, v in t.items() if k != "pixels"})
