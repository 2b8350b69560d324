"""CPU: which scene descriptions sdmm_scene_create and the *_host entry points
accept, and the message each rejection carries -- a table of small
descriptions (the Cornell box at 32 x 18 and one with a cube as 12 triangles),
each with one thing wrong and the whole message it must raise; a few with two
things wrong pin the order of the checks.

Validation comes before anything touches the device, so a rejection is
SDMM_E_INVALID (-1) with its message everywhere.  An accepted description
goes on to the device: without one the call fails with the HIP code (-2),
with one it succeeds -- both count as accepted here.
"""
import copy

import numpy as np
import pytest

F32 = np.float32
NAN, INF = F32(np.nan), F32(np.inf)
TINY = F32(2.0 ** -126)                      # the smallest normal float: "just outside" a bound at 0
ABOVE1, ABOVE2 = np.nextafter(F32(1), F32(3)), np.nextafter(F32(2), F32(3))
BELOW1, BELOW2 = np.nextafter(F32(1), F32(0)), np.nextafter(F32(2), F32(0))
BIG = F32(3e38)                              # finite; two of them sum to inf

CREATE = "sdmm_scene_create"
BAD_PARAMS = "invalid bsdf_params"
BAD_TRANS = "invalid bsdf_params (a smooth dielectric's transmittance is negative or not finite)"
BAD_LEARNED = "learned model with a non-finite value, a negative weight or a non-unit direction"
BAD_M4 = "invalid learned model (1 <= M <= 8, arrays)"
BAD_MND = "invalid learned model (C 2 or 3, 1 <= M <= 8, arrays)"
PHONG_ND = "a Phong BSDF's learned model needs C = 3 and M >= 2"
DIEL_ND = "a rough dielectric's learned model needs C = 3"
TWO_ENTRY = "a bsdf_twosided entry other than 0 or 1"
TWO_KIND = "bsdf_twosided on a transmitting BSDF (kind 4 or 5)"

# one BSDF of every kind (bsdf_params kinds 1 .. 6; the others stay diffuse)
KINDS = {1: "Floor", 2: "TallBox", 3: "ShortBox", 4: "LeftWall", 5: "RightWall", 6: "BackWall"}


@pytest.fixture(scope="module")
def base(scenes):
    """(names, the all-kinds Cornell box, the box with the short cube as triangles)."""
    names = list(scenes._BSDFS)
    box = scenes.cornell_box(32, 18, plastic=(KINDS[1],), conductor=(KINDS[2],), phong=(KINDS[3],),
                             dielectric=(KINDS[4],), glass=(KINDS[5],), mirror=(KINDS[6],))
    bp = box["bsdf_params"].reshape(-1, 8)
    assert [bp[names.index(KINDS[k]), 0] for k in range(1, 7)] == [1, 2, 3, 4, 5, 6]
    assert box["learned_models"][names.index(KINDS[2])] is not None
    assert box["learned_models_nd"][names.index(KINDS[3])] is not None
    assert box["learned_models_nd"][names.index(KINDS[4])] is not None
    mesh = scenes.cornell_box(32, 18, mesh=("ShortBox",))
    assert mesh["triangles"].size == 36
    return names, box, mesh


def changed(desc, **kw):
    c = copy.deepcopy(desc)
    for k, v in kw.items():
        if v is None:
            c.pop(k, None)
        else:
            c[k] = v
    return c


def outcome(pkg, call):
    """None: accepted (no error, or the HIP code of a machine without a
    device); otherwise the whole error string."""
    try:
        call()
    except pkg.SDMMError as e:
        return None if str(e).startswith("sdmm error -2: ") else str(e)
    return None


def run_table(pkg, table, call, who=CREATE):
    """table: (label, description, message or None).  Every entry is run; the
    mismatches are reported together."""
    wrong = []
    for label, desc, msg in table:
        want = None if msg is None else f"sdmm error -1: {who}: {msg}"
        got = outcome(pkg, lambda: call(desc))
        if got != want:
            wrong.append(f"{label}: got {got!r}, want {want!r}")
    assert not wrong, "\n".join(wrong)
    return len(table)


def with_param(desc, b, slot, value):
    c = copy.deepcopy(desc)
    c["bsdf_params"][8 * b + slot] = value
    return c


# ---- bsdf_params ----------------------------------------------------------------------
# per kind and slot: (accepted values, rejected values) -- both sides of every
# inequality, NaN and inf in every checked slot
SPEC = ([0.0, -0.0, TINY, 1.0, BIG], [-TINY, -1.0, NAN, INF, -INF])      # slots 1 .. 3 of kinds 2 .. 6
POS_FINITE = ([TINY, 0.5, 1.5, BIG], [0.0, -0.0, -TINY, NAN, INF, -INF])
NONNEG_FINITE = ([0.0, -0.0, TINY, 7.0, BIG], [-TINY, -3.0, NAN, INF, -INF])
ALPHA = ([TINY, 0.2, BELOW2, 2.0], [0.0, -0.0, -0.1, ABOVE2, 3.0, NAN, INF, -INF])
ETA = ([TINY, 0.5, BELOW1, ABOVE1, 1.5, BIG], [1.0, 0.0, -0.0, -1.5, NAN, INF, -INF])
UNIT = ([0.0, -0.0, TINY, 0.5, BELOW1, 1.0], [-TINY, -0.5, ABOVE1, 2.0, NAN, INF, -INF])
SLOTS = {
    # the plastic kind tests no finiteness and leaves its specular triple alone
    1: {1: ([NAN, INF, -1.0], []), 2: ([NAN], []), 3: ([-INF], []),
        4: ([TINY, 1.49, INF], [0.0, -0.0, -1.0, NAN, -INF]),
        5: ([TINY, 0.45, INF], [0.0, -0.0, -1.0, NAN, -INF]),
        6: ([BELOW1, 0.0, -5.0, -INF], [1.0, ABOVE1, NAN, INF]),
        7: ([0.0, -0.0, 0.5, 1.0], [-TINY, ABOVE1, NAN, INF, -INF])},
    2: {1: SPEC, 2: SPEC, 3: SPEC, 4: POS_FINITE, 5: NONNEG_FINITE, 6: ALPHA, 7: ([NAN, -1.0], [])},
    3: {1: SPEC, 2: SPEC, 3: SPEC, 4: NONNEG_FINITE, 5: UNIT, 6: ([NAN], []), 7: ([INF], [])},
    4: {1: SPEC, 2: SPEC, 3: SPEC, 4: ETA, 5: POS_FINITE, 6: ALPHA, 7: ([NAN], [])},
    5: {1: SPEC, 2: SPEC, 3: SPEC, 4: ETA, 5: POS_FINITE, 6: ([NAN, -1.0], []), 7: ([INF], [])},
    6: {1: SPEC, 2: SPEC, 3: SPEC, 4: POS_FINITE, 5: NONNEG_FINITE, 6: ([NAN], []), 7: ([-INF], [])},
}


def test_bsdf_params(pkg, base):
    names, box, _ = base
    table = [("the all-kinds box", box, None)]
    for kind, slots in SLOTS.items():
        b = names.index(KINDS[kind])
        for slot, (good, bad) in slots.items():
            table += [(f"kind {kind} slot {slot} = {v!r}", with_param(box, b, slot, v), None) for v in good]
            table += [(f"kind {kind} slot {slot} = {v!r}", with_param(box, b, slot, v), BAD_PARAMS) for v in bad]
        if kind >= 2:
            # each finite, their float sum is not
            c = with_param(with_param(box, b, 1, BIG), b, 2, BIG)
            table.append((f"kind {kind}: the specular triple sums to inf", c, BAD_PARAMS))
    # a kind that is not one of 0 .. 6; a diffuse row's other slots are not read
    d = names.index("Ceiling")
    for v in (7.0, -1.0, 0.5, 2.5, NAN, INF, 255.0):
        table.append((f"kind {v!r}", with_param(box, d, 0, v), BAD_PARAMS))
    for v in (0.0, -0.0):
        c = with_param(box, d, 0, v)
        c["bsdf_params"][8 * d + 1: 8 * d + 8] = NAN
        table.append((f"kind {v!r} with NaN slots", c, None))
    # the smooth dielectric's transmittance (its reflectance row): checked for kind 5 only
    g = names.index(KINDS[5])
    for ch in range(3):
        for v, msg in ((0.0, None), (-0.0, None), (BIG, None), (-TINY, BAD_TRANS), (NAN, BAD_TRANS),
                       (INF, BAD_TRANS), (-INF, BAD_TRANS)):
            c = changed(box)
            c["reflectance"][3 * g + ch] = v
            table.append((f"kind 5 transmittance[{ch}] = {v!r}", c, msg))
    c = changed(box)
    c["reflectance"][3 * g: 3 * g + 2] = BIG
    table.append(("kind 5 transmittance sums to inf", c, BAD_TRANS))
    for kind in (0, 1, 2, 3, 4, 6):
        c = changed(box)
        c["reflectance"][3 * names.index(KINDS.get(kind, "Ceiling")) + 1] = NAN
        table.append((f"kind {kind}: a NaN reflectance is not looked at", c, None))
    assert run_table(pkg, table, pkg.Scene) > 250


# ---- learned models -------------------------------------------------------------------
def _model(scenes, nd, M=None):
    """The conductor's SDMM4 (nd False) or the Phong SDMM5 (nd True), cut or
    cycled to M components: (weights, means, covs), fresh arrays."""
    w, mu, cv = scenes.load_learned_nd(scenes.LEARNED_PHONG) if nd else scenes.load_learned()
    ix = np.arange(len(w) if M is None else M) % len(w)
    return w[ix].copy(), mu[ix].copy(), cv[ix].copy()


def _learned_cases(pkg, scenes, names, box, nd):
    """(label, description, message) for one of the two tables; the model sits
    on the conductor (SDMM4) or on the Phong BSDF (ND)."""
    key = "learned_models_nd" if nd else "learned_models"
    b = names.index(KINDS[3] if nd else KINDS[2])
    d0 = 3 if nd else 2                                          # the direction's offset in a mean
    tag = "nd" if nd else "sdmm4"

    def put(model, at=b, desc=box):
        c = changed(desc)
        c[key][at] = model
        return c
    table = [(f"{tag}: the file's model", put(_model(scenes, nd)), None),
             (f"{tag}: M = 8", put(_model(scenes, nd, 8)), None),
             (f"{tag}: M = 9", put(_model(scenes, nd, 9)), BAD_MND if nd else BAD_M4)]
    w, mu, cv = _model(scenes, nd)
    for k in (0, len(w) - 1):
        bad = cv.copy()
        bad[k, 5] = NAN
        table.append((f"{tag}: a NaN covariance in component {k}", put((w, mu, bad)), BAD_LEARNED))
        bad = cv.copy()
        bad[k, -1] = INF
        table.append((f"{tag}: an inf covariance in component {k}", put((w, mu, bad)), BAD_LEARNED))
        bad = mu.copy()
        bad[k, 0] = NAN
        table.append((f"{tag}: a NaN condition mean in component {k}", put((w, bad, cv)), BAD_LEARNED))
        for v, msg in ((-0.0, None), (0.0, None), (-TINY, BAD_LEARNED), (-0.25, BAD_LEARNED), (NAN, BAD_LEARNED),
                       (INF, BAD_LEARNED)):
            ww = w.copy()
            ww[k] = v
            table.append((f"{tag}: weight {v!r} in component {k}", put((ww, mu, cv)), msg))
        # |d|^2 - 1 = +-2e-5 is refused, +-2e-6 passes (the bound is 1e-5 on the squared length)
        unit = mu[k, d0:].astype(np.float64)
        unit /= np.linalg.norm(unit)
        for scale, msg in ((1 + 1e-5, BAD_LEARNED), (1 - 1e-5, BAD_LEARNED), (1 + 1e-6, None), (1 - 1e-6, None),
                           (1.5, BAD_LEARNED), (0.0, BAD_LEARNED)):
            bad = mu.copy()
            bad[k, d0:] = (unit * scale).astype(F32)
            n2 = float((bad[k, d0:].astype(np.float64) ** 2).sum())
            assert (abs(n2 - 1) > 1e-5) == (msg is not None) and abs(abs(n2 - 1) - 1e-5) > 5e-6
            table.append((f"{tag}: direction scaled by {scale} in component {k}", put((w, bad, cv)), msg))
        # the slot before the direction is a condition mean: any finite value passes
        ok = mu.copy()
        ok[k, d0 - 1] = 40.0
        table.append((f"{tag}: a far condition mean in component {k}", put((w, ok, cv)), None))
    # M == 0 is skipped; a delta-only kind's entry is neither read nor checked
    garbage = (np.full(9, NAN, F32), np.full((9, 3 + d0), NAN, F32), np.full((9, (2 + d0) ** 2), NAN, F32))
    table.append((f"{tag}: garbage on a diffuse BSDF", put(garbage, names.index("Ceiling")), BAD_MND if nd else BAD_M4))
    for kind in (5, 6):
        table.append((f"{tag}: garbage on kind {kind}", put(garbage, names.index(KINDS[kind])), None))
    empty = (np.zeros(0, F32), np.zeros((0, 3 + d0), F32), np.zeros((0, (2 + d0) ** 2), F32))
    # (an M = 0 model has no row to read C from: the class built by hand)
    table.append((f"{tag}: M = 0", put(pkg.LearnedBSDFND(*empty, C=d0) if nd else pkg.LearnedBSDF(*empty)), None))
    # without bsdf_params every BSDF is diffuse: a model is checked on any of them
    plain = changed(box, bsdf_params=None, learned_models=None, learned_models_nd=None)
    plain[key] = [None] * len(names)
    table.append((f"{tag}: no bsdf_params, a model", put(_model(scenes, nd), names.index(KINDS[5]), plain), None))
    table.append((f"{tag}: no bsdf_params, garbage where kind 5 was", put(garbage, names.index(KINDS[5]), plain),
                  BAD_MND if nd else BAD_M4))
    return table


def test_learned_models(pkg, scenes, base):
    names, box, _ = base
    table = _learned_cases(pkg, scenes, names, box, False) + _learned_cases(pkg, scenes, names, box, True)
    p, di, fl = names.index(KINDS[3]), names.index(KINDS[4]), names.index("Ceiling")
    w4, mu4, cv4 = _model(scenes, False)                        # C = 2 as an ND model
    w5, mu5, cv5 = _model(scenes, True)

    def nd(at, model):
        c = changed(box)
        c["learned_models_nd"][at] = model
        return c
    # C = 4: 7 means and 36 covariances per component
    c4 = pkg.LearnedBSDFND(w5, np.concatenate([mu5[:, :1], mu5], 1), np.zeros((len(w5), 36), F32), C=4)
    c1 = pkg.LearnedBSDFND(w5, mu5[:, 2:], np.zeros((len(w5), 9), F32), C=1)
    table += [("nd: C = 4", nd(fl, c4), BAD_MND), ("nd: C = 1", nd(fl, c1), BAD_MND),
              ("nd: C = 2 on a diffuse BSDF", nd(fl, (w4, mu4, cv4)), None),
              ("nd: C = 2 on a conductor", nd(names.index(KINDS[2]), (w4, mu4, cv4)), None),
              ("nd: C = 3 on a conductor", nd(names.index(KINDS[2]), (w5, mu5, cv5)), None),
              ("nd: Phong with C = 2", nd(p, (w4, mu4, cv4)), PHONG_ND),
              ("nd: Phong with M = 1", nd(p, _model(scenes, True, 1)), PHONG_ND),
              ("nd: Phong with M = 2", nd(p, _model(scenes, True, 2)), None),
              ("nd: rough dielectric with C = 2", nd(di, (w4, mu4, cv4)), DIEL_ND),
              ("nd: rough dielectric with M = 1", nd(di, _model(scenes, True, 1)), None),
              # the shape checks come before the record checks
              ("nd: Phong with C = 4", nd(p, c4), BAD_MND)]
    bad = mu4.copy()
    bad[0, 2:] *= 1.5
    table.append(("nd: Phong with C = 2 and a non-unit direction", nd(p, (w4, bad, cv4)), PHONG_ND))
    assert run_table(pkg, table, pkg.Scene) > 90


# ---- two-sided flags, geometry, the create arguments -----------------------------------
def test_twosided_and_geometry(pkg, scenes, base):
    names, box, mesh = base
    B = len(names)

    def flags(**kw):
        f = np.zeros(B, np.int32)
        for nm, v in kw.items():
            f[names.index(nm)] = v
        return f
    table = [("twosided: all zeros", changed(box, bsdf_twosided=flags()), None),
             ("twosided: kinds 0, 1, 2, 3, 6", changed(box, bsdf_twosided=flags(
                 Ceiling=1, **{KINDS[k]: 1 for k in (1, 2, 3, 6)})), None),
             ("twosided: an entry of 2", changed(box, bsdf_twosided=flags(Ceiling=2)), TWO_ENTRY),
             ("twosided: an entry of -1", changed(box, bsdf_twosided=flags(Ceiling=-1)), TWO_ENTRY),
             ("twosided: kind 4", changed(box, bsdf_twosided=flags(**{KINDS[4]: 1})), TWO_KIND),
             ("twosided: kind 5", changed(box, bsdf_twosided=flags(**{KINDS[5]: 1})), TWO_KIND),
             ("twosided: 2 on kind 4", changed(box, bsdf_twosided=flags(**{KINDS[4]: 2})), TWO_ENTRY),
             # the first bad entry in BSDF order gives the message
             ("twosided: kind 4 before an entry of 2", changed(box, bsdf_twosided=flags(
                 **{names[0]: 1, names[-1]: 2})), TWO_KIND if names[0] == KINDS[4] else TWO_ENTRY),
             # without bsdf_params every BSDF is diffuse
             ("twosided: no bsdf_params", changed(box, bsdf_params=None, learned_models=None, learned_models_nd=None,
                                                  bsdf_twosided=np.ones(B, np.int32)), None)]
    assert names[0] == KINDS[4]
    plain = scenes.cornell_box(32, 18)
    q = plain["quads"].copy()
    q[9 * 4 + 6: 9 * 4 + 9] = q[9 * 4 + 3: 9 * 4 + 6]            # e2 = e1
    q0 = plain["quads"].copy()
    q0[3:6] = 0.0
    qn = plain["quads"].copy()
    qn[3] = NAN
    bs, em = plain["bsdf"].copy(), plain["emitter"].copy()
    table += [("plain box", plain, None), ("mesh box", mesh, None),
              ("degenerate quad (parallel edges)", changed(plain, quads=q), "degenerate quad"),
              ("degenerate quad (a zero edge)", changed(plain, quads=q0), "degenerate quad"),
              ("degenerate quad (NaN)", changed(plain, quads=qn), "degenerate quad")]
    for v, msg in ((B - 1, None), (B, "material index out of range"), (-1, "material index out of range")):
        c = bs.copy()
        c[3] = v
        table.append((f"quad bsdf {v}", changed(plain, bsdf=c), msg))
    for v, msg in ((0, None), (-1, None), (1, "material index out of range"), (-2, "material index out of range")):
        c = em.copy()
        c[2] = v
        table.append((f"quad emitter {v}", changed(plain, emitter=c), msg))
    table += [("emitters without radiance", changed(plain, radiance=None), "emitters without radiance"),
              ("no emitter array, no radiance", changed(plain, radiance=None, emitter=None), None),
              ("tri_emitter without radiance", changed(mesh, radiance=None, emitter=None,
                                                       tri_emitter=np.full(12, -1, np.int32)),
               "emitters without radiance"),
              ("mesh_normals without triangles", changed(plain, mesh_vertices=mesh["mesh_vertices"],
                                                         mesh_normals=np.ones_like(mesh["mesh_vertices"])),
               "mesh_normals without triangles")]
    # the create call's own arguments
    for k, v, msg in (("width", 0, "invalid description"), ("height", 0, "invalid description"),
                      ("width", -4, "invalid description"), ("fov_x_deg", 0.0, "invalid description"),
                      ("fov_x_deg", 180.0, "invalid description"), ("fov_x_deg", NAN, "invalid description"),
                      ("fov_x_deg", -35.0, "invalid description"), ("fov_x_deg", 179.0, None), ("width", 1, None)):
        table.append((f"{k} = {v!r}", changed(plain, **{k: v}), msg))
    table.append(("no primitive at all", changed(plain, quads=None), "invalid description"))
    table.append(("triangles alone", changed(mesh, quads=None, emitter=None), None))
    # the mesh's own checks, through create
    tri = mesh["triangles"].copy()
    tri[4] = mesh["mesh_vertices"].size // 3
    tb = mesh["tri_bsdf"].copy()
    tb[5] = B
    v = mesh["mesh_vertices"].copy()
    v[7] = INF
    nz = np.ones_like(mesh["mesh_vertices"])
    nz[3:6] = 0.0
    table += [("mesh: vertex index", changed(mesh, triangles=tri), "mesh: vertex index out of range"),
              ("mesh: tri_bsdf", changed(mesh, tri_bsdf=tb), "mesh: material index out of range"),
              ("mesh: no tri_bsdf", changed(mesh, tri_bsdf=None), "mesh: tri_bsdf is required with triangles"),
              ("mesh: vertex", changed(mesh, mesh_vertices=v), "mesh: non-finite vertex"),
              ("mesh: vertex normals", changed(mesh, mesh_normals=np.ones_like(mesh["mesh_vertices"])), None),
              ("mesh: a zero vertex normal", changed(mesh, mesh_normals=nz), "mesh: vertex normal of length 0")]
    assert run_table(pkg, table, pkg.Scene) > 40


def _env_cases(good):
    px = good["env_pixels"]
    table = [("env: a map", good, None), ("env: constant", {"env_kind": 1, "env_radiance": [1.0, 0.0, 2.0]}, None),
             ("env_kind 3", {**good, "env_kind": 3}, "env_kind outside 0..2"),
             ("env_kind -1", {**good, "env_kind": -1}, "env_kind outside 0..2"),
             ("a map without pixels", {"env_kind": 2}, "a lat-long environment without env_pixels")]
    for bad in (NAN, INF, F32(-0.5)):
        p = px.copy()
        p[1, 2, 1] = bad
        m = np.eye(3, dtype=F32)
        m[2, 1] = bad
        table += [(f"texel {bad!r}", {**good, "env_pixels": p}, "a non-finite or negative environment texel"),
                  (f"env_scale {bad!r}", {**good, "env_scale": bad}, "a non-finite or negative env_scale"),
                  (f"env_radiance {bad!r}", {"env_kind": 1, "env_radiance": [1.0, 1.0, bad]},
                   "a non-finite or negative env_radiance")]
        if not bad < 0:
            table.append((f"env_world_to_local {bad!r}", {**good, "env_world_to_local": m},
                          "a non-finite env_world_to_local entry"))
    # the scale comes before the matrix, the matrix before the texels
    m = np.eye(3, dtype=F32)
    m[0, 0] = NAN
    p = px.copy()
    p[0, 0, 0] = NAN
    table += [("env: scale and matrix", {**good, "env_scale": NAN, "env_world_to_local": m},
               "a non-finite or negative env_scale"),
              ("env: matrix and texel", {**good, "env_pixels": p, "env_world_to_local": m},
               "a non-finite env_world_to_local entry")]
    return table


def test_env_through_create(pkg, scenes, base):
    _, _, mesh = base
    plain = scenes.cornell_box(32, 18)
    px = np.random.default_rng(3).uniform(0.0, 2.0, (4, 8, 3)).astype(F32)
    good = {"env_kind": 2, "env_pixels": px, "env_scale": 1.5}
    cases = _env_cases(good)
    table = [(label, {**scene, **env}, msg) for label, env, msg in cases for scene in (plain, mesh)]
    assert run_table(pkg, table, pkg.Scene) > 30
    run_table(pkg, cases, lambda d: pkg.env_eval_host(d, np.asarray([[0.0, 1.0, 0.0]], F32)), who="sdmm_env_eval_host")
    # sizes an array's shape cannot express: through the struct
    sd, keep = pkg._SceneDesc(), {}
    pkg._fill_geometry(sd, {**plain, **good}, keep)
    for i, x in enumerate(plain["camera_to_world"]):
        sd.camera_to_world[i] = float(x)
    sd.fov_x_deg, sd.width, sd.height = 35.0, 32, 18

    def create():
        h = pkg.C.c_void_p()
        rc = pkg.lib().sdmm_scene_create(pkg.C.byref(sd), 0, pkg.C.byref(h))
        msg = pkg.lib().sdmm_last_error().decode() if rc else ""
        if h:
            pkg.lib().sdmm_scene_destroy(h)
        return rc, msg
    assert create()[0] in (0, -2)
    for w, h, word in ((0, 4, "env_width or env_height < 1"), (8, 0, "env_width or env_height < 1"),
                       (-8, 4, "env_width or env_height < 1"),
                       (1 << 14, (1 << 12) + 1, "an environment map of more than 2^26 texels")):
        sd.env_width, sd.env_height = w, h
        assert create() == (-1, f"sdmm_scene_create: {word}")
    # NULL out, NULL description
    assert pkg.lib().sdmm_scene_create(pkg.C.byref(sd), 0, None) == -1
    assert pkg.lib().sdmm_last_error().decode() == "sdmm_scene_create: invalid description"
    assert pkg.lib().sdmm_scene_create(None, 0, pkg.C.byref(pkg.C.c_void_p())) == -1


# ---- the order of the checks ----------------------------------------------------------
def test_first_failing_check_gives_the_message(pkg, scenes, base):
    names, box, mesh = base
    B = len(names)
    c2, p3, g5, fl = (names.index(KINDS[2]), names.index(KINDS[3]), names.index(KINDS[5]), names.index("Ceiling"))
    bad_params = with_param(box, c2, 6, 3.0)
    w, mu, cv = _model(scenes, False)
    bad4 = (w, mu, np.full_like(cv, NAN))
    w5, mu5, cv5 = _model(scenes, True)
    bad5 = (w5, mu5, np.full_like(cv5, NAN))
    two = np.zeros(B, np.int32)
    two[fl] = 2
    q = box["quads"].copy()
    q[3:6] = 0.0
    bs = box["bsdf"].copy()
    bs[0] = B
    tri = mesh["triangles"].copy()
    tri[0] = -1
    bad_env = {"env_kind": 5}

    def model(desc, key, at, m):
        c = changed(desc)
        c[key][at] = m
        return c
    trans = changed(box)
    trans["reflectance"][3 * g5] = NAN
    first, later = min(c2, g5), max(c2, g5)
    both = with_param(trans, c2, 6, 3.0)
    table = [
        ("arguments before emitters", changed(box, width=0, radiance=None), "invalid description"),
        ("emitters before bsdf_params", changed(bad_params, radiance=None), "emitters without radiance"),
        ("bsdf_params in BSDF order", both, BAD_PARAMS if first == c2 else BAD_TRANS),
        ("bsdf_params before the learned models", model(bad_params, "learned_models", c2, bad4), BAD_PARAMS),
        ("transmittance before the learned models", model(trans, "learned_models", c2, bad4), BAD_TRANS),
        ("sdmm4 before nd", model(model(box, "learned_models", c2, bad4), "learned_models_nd", p3,
                                  _model(scenes, True, 1)), BAD_LEARNED),
        ("sdmm4 shape before nd", model(model(box, "learned_models", c2, _model(scenes, False, 9)),
                                        "learned_models_nd", p3, bad5), BAD_M4),
        ("nd before the two-sided flags", changed(model(box, "learned_models_nd", p3, _model(scenes, True, 1)),
                                                  bsdf_twosided=two), PHONG_ND),
        ("learned models before the quads", changed(model(box, "learned_models", c2, bad4), quads=q), BAD_LEARNED),
        ("two-sided flags before the quads", changed(box, bsdf_twosided=two, quads=q), TWO_ENTRY),
        ("quads in order", changed(box, quads=q, bsdf=bs), "degenerate quad"),
        ("quads before the environment", changed(box, bsdf=bs, **bad_env), "material index out of range"),
        ("mesh_normals before the two-sided flags", changed(
            box, bsdf_twosided=two, mesh_vertices=mesh["mesh_vertices"],
            mesh_normals=np.ones_like(mesh["mesh_vertices"])), "mesh_normals without triangles"),
        ("quads before the mesh", changed(mesh, quads=_zero_edge(mesh), triangles=tri), "degenerate quad"),
        ("mesh before the environment", changed(mesh, triangles=tri, **bad_env), "mesh: vertex index out of range"),
    ]
    assert later != first
    run_table(pkg, table, pkg.Scene)


def _zero_edge(desc):
    q = desc["quads"].copy()
    q[3:6] = 0.0
    return q


# ---- the *_host entry points ----------------------------------------------------------
def test_host_entry_points(pkg, scenes, base):
    names, box, mesh = base
    B = len(names)
    plain = scenes.cornell_box(32, 18)
    o, d = np.zeros((1, 3), F32), np.asarray([[0.0, 0.0, -1.0]], F32)
    two = np.zeros(B, np.int32)
    two[names.index("Ceiling")] = 2
    two4 = np.zeros(B, np.int32)
    two4[names.index(KINDS[4])] = 1
    tri = mesh["triangles"].copy()
    tri[4] = -1
    area = mesh["triangles"].copy()
    area[3:6] = [2, 2, 3]
    bs = plain["bsdf"].copy()
    bs[1] = -1
    vn = np.ones_like(mesh["mesh_vertices"])
    vn[0] = NAN
    table = [
        ("plain", plain, None), ("mesh", mesh, None), ("all kinds", box, None),
        # bsdf_params, the learned models, the camera and the environment are create's alone
        ("bad bsdf_params", with_param(box, names.index(KINDS[2]), 6, 3.0), None),
        ("width 0", changed(plain, width=0), None), ("env_kind 5", changed(plain, env_kind=5), None),
        ("no primitive", changed(plain, quads=None), "invalid description"),
        ("mesh_normals without triangles", changed(plain, mesh_vertices=mesh["mesh_vertices"],
                                                   mesh_normals=np.ones_like(mesh["mesh_vertices"])),
         "mesh_normals without triangles"),
        ("twosided 2", changed(box, bsdf_twosided=two), TWO_ENTRY),
        ("twosided on kind 4", changed(box, bsdf_twosided=two4), TWO_KIND),
        ("emitters without radiance", changed(plain, radiance=None), "emitters without radiance"),
        ("degenerate quad", changed(plain, quads=_zero_edge(plain)), "degenerate quad"),
        ("material index", changed(plain, bsdf=bs), "material index out of range"),
        ("vertex index", changed(mesh, triangles=tri), "mesh: vertex index out of range"),
        ("zero-area triangle", changed(mesh, triangles=area), "mesh: zero-area triangle"),
        ("vertex normal", changed(mesh, mesh_normals=vn), "mesh: non-finite vertex normal"),
        ("no tri_bsdf", changed(mesh, tri_bsdf=None), "mesh: tri_bsdf is required with triangles"),
        ("no vertices", changed(mesh, mesh_vertices=None),
         "mesh: vertices and triangles needed (at most 2^26 triangles)"),
        # in order: the arguments, mesh_normals, the flags, the emitters, the quads, the mesh
        ("flags before the quads", changed(box, bsdf_twosided=two, quads=_zero_edge(box)), TWO_ENTRY),
        ("emitters before the quads", changed(plain, radiance=None, quads=_zero_edge(plain)),
         "emitters without radiance"),
        ("quads before the mesh", changed(mesh, quads=_zero_edge(mesh), triangles=tri), "degenerate quad"),
    ]
    n = run_table(pkg, table, lambda c: pkg.intersect_host(c, o, d), who="sdmm_scene_intersect_host")
    assert n == run_table(pkg, table, lambda c: pkg.shading_host(c, o, d), who="sdmm_scene_shading_host")
    # the calls' own arguments come before the description
    bad = changed(plain, quads=_zero_edge(plain))
    for mode in (2, -1):
        assert outcome(pkg, lambda: pkg.intersect_host(bad, o, d, mode=mode)) == \
            "sdmm error -1: sdmm_scene_intersect_host: invalid argument (mode 0 or 1)"
        assert outcome(pkg, lambda: pkg.shading_host(bad, o, d, mode=mode)) == \
            "sdmm error -1: sdmm_scene_shading_host: invalid argument (mode 0 or 1)"
    assert outcome(pkg, lambda: pkg.intersect_host(bad, o, d, max_levels=-1)) == \
        "sdmm error -1: sdmm_scene_intersect_host: invalid argument (mode 0 or 1)"
    # no rays: the description is validated all the same
    none = np.zeros((0, 3), F32)
    assert outcome(pkg, lambda: pkg.intersect_host(bad, none, none)) == \
        "sdmm error -1: sdmm_scene_intersect_host: degenerate quad"
    assert outcome(pkg, lambda: pkg.shading_host(plain, none, none)) is None
    # the BVH dump: triangles needed, and the mesh's checks alone (not the quads')
    assert outcome(pkg, lambda: pkg.mesh_bvh_dump(plain)) == \
        "sdmm error -1: sdmm_mesh_bvh_dump: invalid argument (a description with triangles)"
    assert outcome(pkg, lambda: pkg.mesh_bvh_dump(mesh, max_levels=-1)) == \
        "sdmm error -1: sdmm_mesh_bvh_dump: invalid argument (a description with triangles)"
    assert outcome(pkg, lambda: pkg.mesh_bvh_dump(changed(mesh, triangles=tri))) == \
        "sdmm error -1: sdmm_mesh_bvh_dump: mesh: vertex index out of range"
    assert outcome(pkg, lambda: pkg.mesh_bvh_dump(changed(mesh, quads=_zero_edge(mesh)))) is None
    assert pkg.mesh_bvh_dump(mesh)["order"].size == 12
    # the host answers are what they were: a ray above the cubes meets the back wall
    prim, t = pkg.intersect_host(plain, np.asarray([[0.0, 1.9, 6.8]], F32), d)
    assert prim[0] == 2 and abs(float(t[0]) - 7.8) < 1e-5
    p2, t2, ns, ng = pkg.shading_host(plain, np.asarray([[0.0, 1.9, 6.8]], F32), d)
    assert p2[0] == 2 and t2[0] == t[0] and np.array_equal(ns, ng) and abs(float(ns[0, 2]) - 1.0) < 1e-6
