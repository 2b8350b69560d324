"""Scenes and helpers shared by test_twosided_cases.py (CPU) and
test_gpu_twosided.py (GPU): the mirror twins, the flat sheet in the open, and
the geometry the assertions on saved vertices need."""
import numpy as np

# ---- the mirror twins ------------------------------------------------------------
# Scene A: a probe quad in the plane z = 0 (normal +z) inside a box of six
# emitters of distinct radiances, the camera above it.  Scene B: its mirror
# image in z = 0 with the probe keeping its normal, so that every camera ray
# meets the probe from behind.
FACE_RADIANCE = np.array([[1.0, 0.25, 0.5], [0.5, 2.0, 0.125], [0.75, 0.5, 3.0], [4.0, 1.5, 0.25], [0.125, 1.0, 2.5],
                          [2.0, 3.0, 1.0]], np.float32)
PROBE = 6                     # the probe's quad id (after the six faces)
TWIN_KINDS = (0, 1, 2, 3, 6)
TWIN_W = TWIN_H = 32


def _look_from(pos, target):
    pos, target = np.asarray(pos, np.float64), np.asarray(target, np.float64)
    fwd = (target - pos) / np.linalg.norm(target - pos)
    right = np.cross([0.0, 1.0, 0.0], fwd)
    right /= np.linalg.norm(right)
    up = np.cross(fwd, right)
    return np.concatenate([np.stack([right, up, fwd, pos], 1).reshape(-1), [0, 0, 0, 1]]).astype(np.float32)


def probe_material(scenes, kind):
    """(bsdf_params row, reflectance row) of the probe for a BSDF kind."""
    rho = (0.7, 0.5, 0.3)
    if kind == 0:
        return np.zeros(8, np.float32), np.asarray(rho, np.float32)
    if kind == 1:
        return scenes.plastic_params(rho), np.asarray(rho, np.float32)
    if kind == 2:
        return scenes.conductor_params((0.9, 0.8, 0.7), alpha=0.3), np.zeros(3, np.float32)
    if kind == 3:
        return scenes.phong_params((0.5, 0.4, 0.3), (0.4, 0.4, 0.4), 20.0)
    if kind == 6:
        return scenes.smooth_conductor_params((0.9, 0.8, 0.7)), np.zeros(3, np.float32)
    raise ValueError(kind)


def twin_scenes(scenes, kind, w=TWIN_W, h=TWIN_H):
    """(A, B): B = mirror_z(A, keep=probe) with bsdf_twosided = 1 on the probe
    (B only).  The camera sits off every axis and every coordinate plane, so
    no ray direction has an exactly zero component; a 30 degree field of view
    keeps every pixel on the probe."""
    cube = np.array([[3.0, 0, 0, 0], [0, 3.0, 0, 0], [0, 0, 3.0, 0]])
    quads = [np.concatenate(f) for f in scenes._cube_faces(cube)]
    quads.append(np.array([-1.0, -1.0, 0.0, 2.0, 0, 0, 0, 2.0, 0]))           # e1 x e2 = +z
    bp, refl = probe_material(scenes, kind)
    A = {"quads": np.asarray(quads, np.float32).reshape(-1), "flip_normals": np.asarray([1] * 6 + [0], np.int32),
         "bsdf": np.asarray([0] * 6 + [1], np.int32),
         "reflectance": np.concatenate([np.zeros(3, np.float32), refl]).astype(np.float32),
         "emitter": np.asarray(list(range(6)) + [-1], np.int32), "radiance": FACE_RADIANCE.reshape(-1).copy(),
         "camera_to_world": _look_from((0.37, 0.53, 2.1), (0.05, -0.07, 0.0)), "fov_x_deg": 30.0, "near_clip": 1e-2,
         "width": w, "height": h, "bsdf_params": np.concatenate([np.zeros(8, np.float32), bp]).astype(np.float32)}
    B = scenes.mirror_z(A, keep=(PROBE,))
    B["bsdf_twosided"] = np.asarray([0, 1], np.int32)
    return A, B


def camera_rays(desc):
    """The camera kernel's rays through the pixel centres: (o, d) float32 [n, 3]."""
    W, H = desc["width"], desc["height"]
    cam = np.asarray(desc["camera_to_world"], np.float64).reshape(4, 4)[:3]
    tanx = np.tan(0.5 * np.radians(desc["fov_x_deg"]))
    SX, SY = np.meshgrid((np.arange(W) + 0.5) / W, (np.arange(H) + 0.5) / H)
    l = np.stack([(1 - 2 * SX) * tanx, (1 - 2 * SY) * tanx / (W / H), np.ones_like(SX)], -1).reshape(-1, 3)
    d = l @ cam[:, :3].T
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = np.broadcast_to(cam[:, 3], d.shape)
    return np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)


# ---- the flat sheet in the open ----------------------------------------------------
SHEET_RHO = (0.625, 0.5, 0.375)
SHEET_L = (1.5, 2.25, 0.75)
SHEET_N = np.array([0.0, 1.0, 0.0])


def flat_sheet(scenes, twosided=True, w=48, h=27):
    """A flat diffuse sheet y = 0 of two cells under a constant environment and
    nothing else: the cell x < 0 wound with its normal up (the camera, above,
    sees its front), the cell x > 0 wound the other way (its back).  Every
    bounce ray leaves the scene, so a sheet pixel at spp 1 is rho * L."""
    v = np.array([[-2, 0, -1.5], [0, 0, -1.5], [2, 0, -1.5], [-2, 0, 1.5], [0, 0, 1.5], [2, 0, 1.5]], np.float32)
    tris = np.array([[0, 3, 4], [0, 4, 1],        # normal +y
                     [1, 5, 4], [1, 2, 5]], np.int32)   # normal -y
    d = {"reflectance": np.asarray(SHEET_RHO, np.float32), "mesh_vertices": v.reshape(-1), "triangles": tris.reshape(-1),
         "tri_bsdf": np.zeros(4, np.int32), "camera_to_world": _look_from((0.3, 2.5, 3.0), (0.0, 0.0, 0.0)),
         "fov_x_deg": 60.0, "near_clip": 1e-2, "width": w, "height": h, **scenes.constant_environment(SHEET_L)}
    if twosided:
        d["bsdf_twosided"] = np.ones(1, np.int32)
    return d


# ---- saved vertices ------------------------------------------------------------------
def vertex_table(rec, nv, V, smin, snorm):
    """The saved vertices of a render as rows: (world position [n, 3] float64,
    wo [n, 3], normal [n, 3])."""
    P = nv.shape[0]
    r = rec.reshape(16, V, P)
    sel = np.arange(V)[:, None] < nv[None, :]
    c = np.stack([r[7 + a][sel] for a in range(3)], 1).astype(np.float64)
    wo = np.stack([r[10 + a][sel] for a in range(3)], 1)
    n = np.stack([r[13 + a][sel] for a in range(3)], 1)
    return c * float(snorm) + np.asarray(smin, np.float64), wo, n


def on_sheet(desc, p, tol=2e-3):
    """Which points lie on sheet_scene's sheet: a height field over z alone,
    piecewise linear between its rows of vertices."""
    v = np.asarray(desc["mesh_vertices"], np.float64).reshape(-1, 3)
    z, idx = np.unique(v[:, 2], return_index=True)
    y = v[idx, 1]
    inside = (p[:, 0] >= v[:, 0].min() - tol) & (p[:, 0] <= v[:, 0].max() + tol) & (p[:, 2] >= z[0] - tol) & \
             (p[:, 2] <= z[-1] + tol)
    return inside & (np.abs(p[:, 1] - np.interp(p[:, 2], z, y)) < tol)


def quad_sides(desc, p, n, tol=2e-3):
    """For vertices (position p, saved normal n) of a scene of quads: +1 where
    the saved normal is the face normal of the quad the point lies on, -1 where
    it is the negated one, 0 where no quad matches."""
    q = np.asarray(desc["quads"], np.float64).reshape(-1, 3, 3)
    p0, e1, e2 = q[:, 0], q[:, 1], q[:, 2]
    fn = np.cross(e1, e2)
    fn /= np.linalg.norm(fn, axis=1)[:, None]
    fn *= np.where(np.asarray(desc.get("flip_normals", np.zeros(len(q))), bool), -1.0, 1.0)[:, None]
    r = p[:, None] - p0[None]                                                   # [m, q, 3]
    a = (r * e1[None]).sum(-1) / (e1 * e1).sum(-1)[None]                        # (rectangles)
    b = (r * e2[None]).sum(-1) / (e2 * e2).sum(-1)[None]
    on = (np.abs((r * fn[None]).sum(-1)) < tol) & (a > -tol) & (a < 1 + tol) & (b > -tol) & (b < 1 + tol)
    cos = n.astype(np.float64) @ fn.T
    side = np.zeros(len(p), np.int32)
    side[(on & (cos > 0.9999)).any(1)] = 1
    side[(on & (cos < -0.9999)).any(1) & (side == 0)] = -1
    return side
