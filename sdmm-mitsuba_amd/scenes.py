"""Analytic scenes for the device Li (sdmm_scene_* in include/sdmm_gpu.h).

cornell_box(): the test suite's Cornell Box, test-suite/scenes/cornell-box/
cornell-box.xml -- film 640x360 (:26-28), perspective fov 35 along x with the
toWorld of :17-19, five rectangles (:75-116; flipNormals on the back, right
and left walls), two cubes (:118-132), the area light (:134-143) and the
diffuse reflectances of :36-73.  The integrator settings of the suite's
_integrators/sdmm.xml: maxDepth = rrDepth = 10.

Mitsuba shapes as parallelograms: a rectangle is [-1, 1]^2 x {0} under
toWorld (normal +z), a cube [-1, 1]^3 (outward normals), both transformed by
the 4x4 matrix of the XML (row major).

The emitter's spectrum "400:0, 500:1600, 600:3180, 700:3680" (piecewise
linear) is converted to linear sRGB here: integrated against the CIE 1931
2-degree observer (the analytic multi-lobe fit of Wyman, Sloan and Shirley,
JCGT 2013) over 360-830 nm, normalised by the integral of y-bar, then XYZ ->
linear sRGB (D65).  Mitsuba's own RGB-mode conversion is not reproducible
here (no Mitsuba); the image is therefore not compared with Mitsuba renders --
the device Li is checked for unbiasedness and its training batches for
parity with the host-routed reference instead (tests/test_gpu_li.py).
"""
import json
from pathlib import Path

import numpy as np

CORNELL_MAX_DEPTH = 10       # _integrators/sdmm.xml: maxDepth
CORNELL_RR_DEPTH = 10        # rrDepth = maxDepth

_RECTS = [
    # (matrix row major 3x4, bsdf, flipNormals)
    ("-4.37114e-008 1 4.37114e-008 0 0 -8.74228e-008 2 0 1 4.37114e-008 1.91069e-015 0", "Floor", False),
    ("-1 7.64274e-015 -1.74846e-007 0 8.74228e-008 8.74228e-008 -2 2 0 -1 -4.37114e-008 0", "Ceiling", False),
    ("1.91069e-015 1 1.31134e-007 0 1 3.82137e-015 -8.74228e-008 1 -4.37114e-008 1.31134e-007 -2 -1",
     "BackWall", True),
    ("4.37114e-008 -1.74846e-007 2 1 1 3.82137e-015 -8.74228e-008 1 3.82137e-015 1 2.18557e-007 0",
     "RightWall", True),
    ("-4.37114e-008 8.74228e-008 -2 -1 1 3.82137e-015 -8.74228e-008 1 0 -1 -4.37114e-008 0", "LeftWall", True),
]
_CUBES = [
    ("0.0851643 0.289542 1.31134e-008 0.328631 3.72265e-009 1.26563e-008 -0.3 0.3 "
     "-0.284951 0.0865363 5.73206e-016 0.374592", "ShortBox"),
    ("0.286776 0.098229 -2.29282e-015 -0.335439 -4.36233e-009 1.23382e-008 -0.6 0.6 "
     "-0.0997984 0.282266 2.62268e-008 -0.291415", "TallBox"),
]
_LIGHT = ("4.700000e-02 -3.322060e-09 -1.561370e-09 -5.000000e-03 -4.108880e-09 7.806860e-10 -1.786000e-02 "
          "1.980000e+00 4.108880e-09 3.800000e-02 1.661032e-09 -3.000000e-02")
_BSDFS = {
    "LeftWall": (0.63, 0.065, 0.05), "RightWall": (0.14, 0.45, 0.091), "Floor": (0.725, 0.71, 0.68),
    "Ceiling": (0.725, 0.71, 0.68), "BackWall": (0.725, 0.71, 0.68), "ShortBox": (0.725, 0.71, 0.68),
    "TallBox": (0.725, 0.71, 0.68), "Light": (0.0, 0.0, 0.0),
}
_LIGHT_SPD = [(400.0, 0.0), (500.0, 1600.0), (600.0, 3180.0), (700.0, 3680.0)]
_CAMERA = "-1 0 0 0 0 1 0 1 0 0 -1 6.8 0 0 0 1"


def _mat(s):
    return np.array([float(x) for x in s.split()], np.float64).reshape(3, 4)


def _cie_xyz(lam):
    """CIE 1931 colour matching functions, multi-lobe analytic fit (Wyman et al. 2013)."""
    def g(x, mu, s1, s2):
        s = np.where(x < mu, s1, s2)
        return np.exp(-0.5 * ((x - mu) / s) ** 2)
    x = 1.056 * g(lam, 599.8, 37.9, 31.0) + 0.362 * g(lam, 442.0, 16.0, 26.7) - 0.065 * g(lam, 501.1, 20.4, 26.2)
    y = 0.821 * g(lam, 568.8, 46.9, 40.5) + 0.286 * g(lam, 530.9, 16.3, 31.1)
    z = 1.217 * g(lam, 437.0, 11.8, 36.0) + 0.681 * g(lam, 459.0, 26.0, 13.8)
    return x, y, z


def spectrum_to_rgb(spd):
    """Piecewise-linear SPD (wavelength, value) -> linear sRGB (zero outside the samples)."""
    lam = np.arange(360.0, 831.0, 1.0)
    w, v = zip(*spd)
    s = np.interp(lam, w, v, left=0.0, right=0.0)
    xb, yb, zb = _cie_xyz(lam)
    X, Y, Z = (np.sum(s * xb), np.sum(s * yb), np.sum(s * zb))
    k = 1.0 / np.sum(yb)
    X, Y, Z = X * k, Y * k, Z * k
    m = np.array([[3.240479, -1.537150, -0.498535], [-0.969256, 1.875991, 0.041556],
                  [0.055648, -0.204043, 1.057311]])
    return np.maximum(m @ np.array([X, Y, Z]), 0.0)


def _rect(M):
    """Corner and edges with e1 x e2 along Mitsuba's normal (inverse transpose of +z)."""
    A, t = M[:, :3], M[:, 3]
    p0 = A @ np.array([-1.0, -1.0, 0.0]) + t
    e1, e2 = A @ np.array([2.0, 0.0, 0.0]), A @ np.array([0.0, 2.0, 0.0])
    return (p0, e2, e1) if np.linalg.det(A) < 0 else (p0, e1, e2)


def _cube_faces(M):
    A, t = M[:, :3], M[:, 3]
    flip = np.linalg.det(A) < 0
    faces = []
    for ax in range(3):
        b, c = (ax + 1) % 3, (ax + 2) % 3
        for s in (1.0, -1.0):
            u = np.zeros(3); u[b] = 2.0
            v = np.zeros(3); v[c] = 2.0
            if (s < 0) != flip:                 # u x v must point along s e_ax after the transform
                u, v = v, u
            corner = np.zeros(3); corner[ax] = s
            corner -= 0.5 * u + 0.5 * v
            faces.append((A @ corner + t, A @ u, A @ v))
    return faces


def _fresnel_dielectric(cos_i, eta):
    """fresnelDielectricExt (libcore/util.cpp:651-681), reflectance only (float64)."""
    if eta == 1.0:
        return 0.0
    scale = 1.0 / eta if cos_i > 0 else eta
    ct2 = 1.0 - (1.0 - cos_i * cos_i) * scale * scale
    if ct2 <= 0.0:
        return 1.0
    ci, ct = abs(cos_i), np.sqrt(ct2)
    rs = (ci - eta * ct) / (ci + eta * ct)
    rp = (eta * ci - ct) / (eta * ci + ct)
    return 0.5 * (rs * rs + rp * rp)


def plastic_params(diffuse_rgb, specular_rgb=(1.0, 1.0, 1.0), int_ior=1.49, ext_ior=1.000277):
    """The 8 bsdf_params floats of a smooth plastic (bsdfs/plastic.cpp:148-200;
    include/sdmm_gpu.h sdmm_scene_desc): kind 1, specularReflectance, eta =
    intIOR / extIOR (polypropylene / air, the plugin's defaults), 1 / eta^2,
    fdrInt = fresnelDiffuseReflectance(1 / eta) (the integral over xi of
    F(sqrt(xi)), here by adaptive quadrature in double where Mitsuba runs a
    Gauss-Lobatto rule: the constant may differ in its last float bits), and
    the specular sampling weight sAvg / (dAvg + sAvg) from the luminances."""
    from scipy.integrate import quad
    f32 = np.float32
    eta = f32(f32(int_ior) / f32(ext_ior))
    inv_eta2 = f32(f32(1.0) / f32(eta * eta))
    fdr_int, _ = quad(lambda xi: _fresnel_dielectric(np.sqrt(xi), 1.0 / float(eta)), 0.0, 1.0,
                      epsabs=1e-12, epsrel=1e-12, limit=200)

    def lum(c):
        c = [f32(x) for x in c]
        return f32(f32(f32(c[0] * f32(0.212671)) + f32(c[1] * f32(0.715160))) + f32(c[2] * f32(0.072169)))
    d_avg, s_avg = lum(diffuse_rgb), lum(specular_rgb)
    ssw = f32(s_avg / f32(d_avg + s_avg))
    return np.array([1.0, *specular_rgb, eta, inv_eta2, fdr_int, ssw], np.float32)


def conductor_params(specular_rgb=(1.0, 1.0, 1.0), eta=1.2, k=7.0, alpha=0.2):
    """The 8 bsdf_params floats of a rough conductor (bsdfs/roughconductor.cpp;
    include/sdmm_gpu.h sdmm_scene_desc): kind 2, specularReflectance, a gray
    eta / k (default: aluminium-like, |n + ik| of Al over the visible), the
    isotropic Beckmann alpha (sampleVisible = false)."""
    return np.array([2.0, *specular_rgb, eta, k, alpha, 0.0], np.float32)


def phong_params(diffuse_rgb, specular_rgb=(0.2, 0.2, 0.2), exponent=30.0):
    """(the 8 bsdf_params floats of a Phong BSDF, its diffuse reflectance)
    after Phong::configure() (bsdfs/phong.cpp:127-156; include/sdmm_gpu.h
    sdmm_scene_desc): kind 3, specularReflectance, the exponent and the
    specular sampling weight sAvg / (dAvg + sAvg) from the luminances; both
    reflectances scaled by 0.99 / max when their channel-wise sum exceeds 1
    (ensureEnergyConservation, librender/bsdf.cpp:115-146)."""
    f32 = np.float32
    d = np.asarray(diffuse_rgb, f32)
    sp = np.asarray(specular_rgb, f32)
    actual_max = f32((d + sp).max())
    if actual_max > 1.0:
        scale = f32(f32(0.99) * f32(f32(1.0) / actual_max))
        d, sp = (d * scale).astype(f32), (sp * scale).astype(f32)

    def lum(c):
        return f32(f32(f32(c[0] * f32(0.212671)) + f32(c[1] * f32(0.715160))) + f32(c[2] * f32(0.072169)))
    d_avg, s_avg = lum(d), lum(sp)
    ssw = f32(s_avg / f32(d_avg + s_avg))
    return np.array([3.0, *sp, exponent, ssw, 0.0, 0.0], f32), d


def checker_texture(w, h, a=(0.8, 0.8, 0.8), b=(0.1, 0.1, 0.1), **fields):
    """A texture (a dict for the description's "textures") of w x h texels,
    texel (x, y) colour a where x + y is even and b where it is odd; nearest
    filter, repeat wrap.  fields: further entries ("filter", "wrap_u",
    "wrap_v", "uv_scale", "uv_offset") or overrides."""
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    px = np.where(((x + y) % 2 == 0)[..., None], np.asarray(a, np.float32), np.asarray(b, np.float32))
    return {"pixels": np.ascontiguousarray(px, np.float32), "filter": "nearest", "wrap_u": "repeat",
            "wrap_v": "repeat", **fields}


def ramp_texture(w, h, **fields):
    """A texture of w x h texels whose red grows with x, green with y (both
    from 0.1 to 0.9 over the texel centres) and whose blue is 0.5; bilinear
    filter, clamp wrap.  fields: as checker_texture's."""
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    r = 0.1 + 0.8 * (x / max(1, w - 1))
    g = 0.1 + 0.8 * (y / max(1, h - 1))
    px = np.stack([r, g, np.full_like(r, 0.5)], -1)
    return {"pixels": np.ascontiguousarray(px, np.float32), "filter": "bilinear", "wrap_u": "clamp",
            "wrap_v": "clamp", **fields}


def texture_mean(texture):
    """The texture's average colour (Texture::getAverage of a bitmap: the mean
    over its texels), float32 [3]: what Phong::configure() and
    SmoothPlastic::configure() take for the diffuse part of their specular
    sampling weight and energy scaling (phong.cpp:146-148, plastic.cpp:
    159-175) -- pass it as the diffuse_rgb of phong_params / plastic_params
    for a BSDF whose reflectance is this texture; the constant bsdf_params
    stay the caller's."""
    return np.asarray(texture["pixels"], np.float64).reshape(-1, 3).mean(0).astype(np.float32)


def dielectric_params(specular_rgb=(1.0, 1.0, 1.0), transmittance_rgb=(1.0, 1.0, 1.0), int_ior=1.5046,
                      ext_ior=1.000277, alpha=0.1):
    """(the 8 bsdf_params floats of a rough dielectric, its
    specularTransmittance -- the BSDF's `reflectance` row)
    (bsdfs/roughdielectric.cpp:213-241; include/sdmm_gpu.h sdmm_scene_desc):
    kind 4, specularReflectance, eta = intIOR / extIOR (bk7 / air, the
    plugin's defaults) and 1 / eta in float, the isotropic Beckmann alpha
    (sampleVisible = false).  Both spectra must lie in [0, 1]
    (ensureEnergyConservation would rescale them otherwise)."""
    f32 = np.float32
    sp, tr = np.asarray(specular_rgb, f32), np.asarray(transmittance_rgb, f32)
    if sp.min() < 0 or sp.max() > 1 or tr.min() < 0 or tr.max() > 1:
        raise ValueError("specular reflectance / transmittance outside [0, 1]")
    if not (int_ior > 0 and ext_ior > 0 and int_ior != ext_ior):
        raise ValueError("the interior and exterior indices of refraction must be positive and differ")
    eta = f32(f32(int_ior) / f32(ext_ior))
    inv_eta = f32(f32(1.0) / eta)
    return np.array([4.0, *sp, eta, inv_eta, alpha, 0.0], f32), tr


def smooth_dielectric_params(specular_rgb=(1.0, 1.0, 1.0), transmittance_rgb=(1.0, 1.0, 1.0), int_ior=1.5046,
                             ext_ior=1.000277):
    """(the 8 bsdf_params floats of a smooth dielectric, its
    specularTransmittance -- the BSDF's `reflectance` row)
    (bsdfs/dielectric.cpp; include/sdmm_gpu.h sdmm_scene_desc): kind 5,
    specularReflectance, eta = intIOR / extIOR (bk7 / air, the plugin's
    defaults) and 1 / eta in float.  A delta-only BSDF: reflection with the
    Fresnel probability, refraction otherwise.  Both spectra must lie in
    [0, 1]."""
    bp, tr = dielectric_params(specular_rgb, transmittance_rgb, int_ior, ext_ior, alpha=0.0)
    bp[0] = 5.0
    return bp, tr


def smooth_conductor_params(specular_rgb=(1.0, 1.0, 1.0), eta=1.2, k=7.0):
    """The 8 bsdf_params floats of a smooth conductor (bsdfs/conductor.cpp;
    include/sdmm_gpu.h sdmm_scene_desc): kind 6, specularReflectance and a
    gray eta / k, the convention of conductor_params (default:
    aluminium-like).  A delta-only BSDF: a one-sided mirror tinted by
    fresnelConductorExact."""
    return np.array([6.0, *specular_rgb, eta, k, 0.0, 0.0], np.float32)


LEARNED_CONDUCTOR = Path(__file__).resolve().parent / "data" / "conductor_beckmann_4c.sdmm4.json"


def load_learned(path=LEARNED_CONDUCTOR):
    """A learned BSDF file (sdmm-amd.sdmm4 JSON, include/sdmm_gpu.h
    sdmm_learned4_load_json) as (weights[M], means[M][5], covs[M][16])
    float32 -- the numbers are written with 9 digits, so they round-trip."""
    doc = json.loads(Path(path).read_text())
    if doc.get("format") != "sdmm-amd.sdmm4" or doc.get("version") != 1:
        raise ValueError(f"{path}: not an sdmm-amd.sdmm4 file")
    M = int(doc["M"])
    return (np.asarray(doc["weights"], np.float32).reshape(M), np.asarray(doc["means"], np.float32).reshape(M, 5),
            np.asarray(doc["covs"], np.float32).reshape(M, 16))


LEARNED_PHONG = Path(__file__).resolve().parent / "data" / "phong_4c.sdmm5.json"


LEARNED_DIELECTRIC = Path(__file__).resolve().parent / "data" / "dielectric_4c.sdmm5.json"


def load_learned_nd(path=LEARNED_PHONG):
    """A learned BSDF over a C-dimensional condition (sdmm-amd.sdmm5 JSON,
    include/sdmm_gpu.h sdmm_learned_load_json; an sdmm-amd.sdmm4 file is C =
    2) as (weights[M], means[M][C+3], covs[M][(C+2)^2]) float32."""
    doc = json.loads(Path(path).read_text())
    fmt = doc.get("format")
    if fmt not in ("sdmm-amd.sdmm5", "sdmm-amd.sdmm4") or doc.get("version") != 1:
        raise ValueError(f"{path}: not an sdmm-amd.sdmm5 file")
    C = int(doc["C"]) if fmt == "sdmm-amd.sdmm5" else 2
    M = int(doc["M"])
    return (np.asarray(doc["weights"], np.float32).reshape(M),
            np.asarray(doc["means"], np.float32).reshape(M, C + 3),
            np.asarray(doc["covs"], np.float32).reshape(M, (C + 2) ** 2))


def cornell_box(width=640, height=360, plastic=(), conductor=(), alpha=0.2, learned=LEARNED_CONDUCTOR, phong=(),
                phong_learned=LEARNED_PHONG, phong_specular=(0.4, 0.4, 0.4), phong_exponent=30.0, dielectric=(),
                dielectric_learned=LEARNED_DIELECTRIC, dielectric_alpha=0.1, dielectric_ior=(1.5046, 1.000277),
                dielectric_specular=(1.0, 1.0, 1.0), dielectric_transmittance=(1.0, 1.0, 1.0), dielectric_lift=0.0,
                mesh=(), glass=(), mirror=(), mirror_eta_k=(1.2, 7.0), twosided=(), textured=False):
    """sdmm_scene_desc fields for the Cornell Box (numpy arrays).  plastic:
    names of BSDFs (e.g. "TallBox", "ShortBox", "Floor") rendered as smooth
    plastic over their diffuse reflectance (a delta specular lobe beside a
    smooth one, like the Kitchen's `plastic` materials, kitchen.xml);
    conductor: names rendered as rough conductors (the Kitchen's glossy
    `roughconductor` materials) tinted by their reflectance, Beckmann alpha,
    each with the learned BSDF `learned` (an sdmm4 file; None: no learned
    model, so product sampling falls back to the plain conditional there) --
    the synthetic stand-in of tools/make_learned_conductor.py by default.
    phong: names rendered as Phong BSDFs (the Kitchen's most common learned
    material) over their diffuse reflectance with phong_specular /
    phong_exponent, each with the learned SDMM5 `phong_learned` (None: no
    model) -- the stand-in of tools/make_learned_phong.py by default.
    dielectric: names rendered as rough dielectrics (the Kitchen's
    `roughdielectric` glass) with dielectric_specular / _transmittance /
    _alpha / _ior = (intIOR, extIOR), each with the learned SDMM5
    `dielectric_learned` (None: no model) -- the stand-in of
    tools/make_learned_dielectric.py by default.  dielectric_lift raises a
    dielectric cube by that much along y: the cubes stand on the floor, and a
    glass box's bottom face would be coplanar with it.  mesh: names of the
    cubes ("ShortBox", "TallBox") given as triangles (quads_to_triangles of
    their faces, the description's mesh fields) instead of quads.
    glass: names rendered as smooth dielectrics (kind 5: the Pool's water and
    glass, the Torus scene's case) with dielectric_specular / _transmittance
    / _ior, a glass cube lifted by dielectric_lift like a rough one; mirror:
    names rendered as smooth conductors (kind 6) tinted by their reflectance
    like `conductor`, with the gray mirror_eta_k = (eta, k).  Neither reads a
    learned model: their bounces are delta only.
    twosided: names wrapped in the single-child `twosided` adapter (the
    description's bsdf_twosided; not a `dielectric` or `glass` name, which
    transmit).  The box is closed, so no path meets such a BSDF from behind.
    textured: a checker (8 x 8 texels of the floor's colour and a dark gray,
    nearest, tiled twice each way) on the floor's reflectance and a ramp (16 x
    16, bilinear, clamped) on the back wall's, which becomes a Phong BSDF
    (phong_specular / phong_exponent, its sampling weight from the ramp's
    mean, the shipped learned SDMM5) -- the description's textures and
    bsdf_texture; quads carry their own (a, b) as uv.  "Floor" and "BackWall"
    then take no other material."""
    names = list(_BSDFS)
    if textured:
        if {"Floor", "BackWall"} & (set(plastic) | set(conductor) | set(phong) | set(dielectric) | set(glass) |
                                    set(mirror)):
            raise ValueError("textured: Floor and BackWall take no other material")
        phong = tuple(phong) + ("BackWall",)
    quads, bsdf, flip, emitter = [], [], [], []
    mesh_quads, mesh_bsdf = [], []
    if set(mesh) - {name for _, name in _CUBES}:
        raise ValueError(f"mesh: only the cubes {[name for _, name in _CUBES]} can be triangles")
    for m, name, fl in _RECTS:
        quads.append(np.concatenate(_rect(_mat(m))))
        bsdf.append(names.index(name)); flip.append(int(fl)); emitter.append(-1)
    for m, name in _CUBES:
        M = _mat(m)
        if name in dielectric or name in glass:
            M[1, 3] += dielectric_lift
        for f in _cube_faces(M):
            if name in mesh:
                mesh_quads.append(np.concatenate(f))
                mesh_bsdf += [names.index(name)] * 2
                continue
            quads.append(np.concatenate(f))
            bsdf.append(names.index(name)); flip.append(0); emitter.append(-1)
    quads.append(np.concatenate(_rect(_mat(_LIGHT))))
    bsdf.append(names.index("Light")); flip.append(0); emitter.append(0)
    cam = np.array([float(x) for x in _CAMERA.split()], np.float32)
    extra = {}
    if mesh_quads:
        v, t = quads_to_triangles(np.asarray(mesh_quads, np.float32))
        extra.update(mesh_vertices=v.reshape(-1), triangles=t.reshape(-1), tri_bsdf=np.asarray(mesh_bsdf, np.int32))
    refl = {n: _BSDFS[n] for n in names}
    if plastic or conductor or phong or dielectric or glass or mirror:
        kinds = [set(plastic), set(conductor), set(phong), set(dielectric), set(glass), set(mirror)]
        unknown = set().union(*kinds) - set(names)
        twice = {n for n in names if sum(n in k for k in kinds) > 1}
        if unknown or twice:
            raise ValueError(f"unknown or doubly assigned BSDFs {sorted(unknown | twice)}")
        bp = np.zeros((len(names), 8), np.float32)
        for i, nm in enumerate(names):
            if nm in plastic:
                bp[i] = plastic_params(_BSDFS[nm])
            elif nm in conductor:
                bp[i] = conductor_params(tuple(min(1.0, 1.25 * c) for c in _BSDFS[nm]), alpha=alpha)
            elif nm in phong:
                bp[i], refl[nm] = phong_params(_BSDFS[nm], phong_specular, phong_exponent)
                if textured and nm == "BackWall":
                    # (the sampling weight from the texture's mean; the row itself is replaced at every hit)
                    bp[i], refl[nm] = phong_params(texture_mean(ramp_texture(16, 16)), phong_specular, phong_exponent)
            elif nm in dielectric:
                bp[i], refl[nm] = dielectric_params(dielectric_specular, dielectric_transmittance, *dielectric_ior,
                                                    alpha=dielectric_alpha)
            elif nm in glass:
                bp[i], refl[nm] = smooth_dielectric_params(dielectric_specular, dielectric_transmittance,
                                                           *dielectric_ior)
            elif nm in mirror:
                bp[i] = smooth_conductor_params(tuple(min(1.0, 1.25 * c) for c in _BSDFS[nm]), *mirror_eta_k)
        extra["bsdf_params"] = bp.reshape(-1)
        if conductor and learned is not None:
            model = load_learned(learned)
            extra["learned_models"] = [model if nm in conductor else None for nm in names]
        if phong and phong_learned is not None:
            model = load_learned_nd(phong_learned)
            extra["learned_models_nd"] = [model if nm in phong else None for nm in names]
        if dielectric and dielectric_learned is not None:
            model = load_learned_nd(dielectric_learned)
            nd = extra.setdefault("learned_models_nd", [None] * len(names))
            extra["learned_models_nd"] = [model if nm in dielectric else cur for nm, cur in zip(names, nd)]
    if twosided:
        bad = (set(twosided) - set(names)) | (set(twosided) & (set(dielectric) | set(glass)))
        if bad:
            raise ValueError(f"twosided: unknown or transmitting BSDFs {sorted(bad)}")
        extra["bsdf_twosided"] = np.asarray([int(nm in twosided) for nm in names], np.int32)
    if textured:
        extra["textures"] = [checker_texture(8, 8, _BSDFS["Floor"], (0.15, 0.15, 0.15), uv_scale=2.0),
                             ramp_texture(16, 16)]
        extra["bsdf_texture"] = np.asarray([{"Floor": 0, "BackWall": 1}.get(nm, -1) for nm in names], np.int32)
    return {**extra,
        "quads": np.asarray(quads, np.float32).reshape(-1),
        "flip_normals": np.asarray(flip, np.int32),
        "bsdf": np.asarray(bsdf, np.int32),
        "reflectance": np.asarray([refl[n] for n in names], np.float32).reshape(-1),
        "emitter": np.asarray(emitter, np.int32),
        "radiance": spectrum_to_rgb(_LIGHT_SPD).astype(np.float32),
        "camera_to_world": cam,
        "fov_x_deg": 35.0,
        "near_clip": 1e-2,
        "width": width,
        "height": height,
    }


def vertex_normals(vertices, triangles):
    """Mitsuba's computeNormals (librender/trimesh.cpp:636-672; Thuermer and
    Wuethrich, "Computing Vertex Normals from Polygonal Facets"): each
    triangle's unit face normal added to its three vertices weighted by the
    triangle's angle there, the sums normalised -- in float64, returned as
    float32 [n_vertices, 3].  A zero-area triangle adds nothing; a vertex no
    triangle reaches gets Mitsuba's bogus (1, 0, 0)."""
    V = np.asarray(vertices, np.float64).reshape(-1, 3)
    T = np.asarray(triangles, np.int64).reshape(-1, 3)
    N = np.zeros_like(V)
    p = V[T]                                                    # [nt, 3, 3]
    fn = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    fl = np.linalg.norm(fn, axis=1)
    ok = fl > 0
    fn[ok] /= fl[ok, None]
    for k in range(3):
        a, b = p[:, (k + 1) % 3] - p[:, k], p[:, (k + 2) % 3] - p[:, k]
        la, lb = np.linalg.norm(a, axis=1), np.linalg.norm(b, axis=1)
        good = ok & (la > 0) & (lb > 0)
        cos = np.zeros(len(T))
        cos[good] = np.einsum("ij,ij->i", a[good], b[good]) / (la[good] * lb[good])
        angle = np.where(good, np.arccos(np.clip(cos, -1.0, 1.0)), 0.0)
        np.add.at(N, T[:, k], fn * angle[:, None])
    ln = np.linalg.norm(N, axis=1)
    bad = ~(ln > 0)
    N[~bad] /= ln[~bad, None]
    N[bad] = (1.0, 0.0, 0.0)
    return N.astype(np.float32)


def torus_mesh(nu, nv, R=1.0, r=0.4, to_world=None, normals=False, uvs=False):
    """A torus about the y axis (centre circle of radius R in the xz plane,
    tube radius r) as nu x nv quads of two triangles: (vertices [nu * nv, 3]
    float32, triangles [2 * nu * nv, 3] int32), counter-clockwise seen from
    outside.  to_world: a 3x4 or 4x4 matrix applied to the vertices.
    normals: also the analytic unit outward normals at the vertices (float32
    [nu * nv, 3], third of the tuple), through to_world's inverse transpose
    and normalised again.  uvs: also the vertices' texture coordinates (i / nu,
    j / nv) (float32 [nu * nv, 2], last of the tuple) -- the ring closes on
    shared vertices, so the last cells along each direction run back from
    (n - 1) / n to 0."""
    u = 2.0 * np.pi * np.arange(nu) / nu
    v = 2.0 * np.pi * np.arange(nv) / nv
    uu, vv = np.meshgrid(u, v, indexing="ij")
    ring = R + r * np.cos(vv)
    P = np.stack([ring * np.cos(uu), r * np.sin(vv), ring * np.sin(uu)], -1).reshape(-1, 3)
    Nn = np.stack([np.cos(vv) * np.cos(uu), np.sin(vv), np.cos(vv) * np.sin(uu)], -1).reshape(-1, 3)
    if to_world is not None:
        M = np.asarray(to_world, np.float64).reshape(-1, 4)[:3]
        P = P @ M[:, :3].T + M[:, 3]
        Nn = Nn @ np.linalg.inv(M[:, :3])       # rows times (A^-T)^T
        Nn /= np.linalg.norm(Nn, axis=1, keepdims=True)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    a = (i * nv + j).reshape(-1)
    b = (((i + 1) % nu) * nv + j).reshape(-1)
    c = (((i + 1) % nu) * nv + (j + 1) % nv).reshape(-1)
    d = (i * nv + (j + 1) % nv).reshape(-1)
    # outward: (dP/dv) x (dP/du) for this parametrisation
    tris = np.concatenate([np.stack([a, d, c], -1), np.stack([a, c, b], -1)], 1).reshape(-1, 3)
    if to_world is not None and np.linalg.det(M[:, :3]) < 0:
        tris = tris[:, ::-1]
    out = (P.astype(np.float32), np.ascontiguousarray(tris, np.int32))
    if normals:
        out += (Nn.astype(np.float32),)
    if uvs:
        out += (np.stack([i / nu, j / nv], -1).reshape(-1, 2).astype(np.float32),)
    return out


def convex_mesh():
    """An octahedron subdivided once and pushed to the unit sphere: (vertices
    [18, 3] float32, triangles [32, 3] int32), counter-clockwise seen from
    outside.  Convex, so no ray leaving it meets it again."""
    V = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    F = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    verts = [np.asarray(v, np.float64) for v in V]
    mid = {}

    def midpoint(i, j):
        key = (min(i, j), max(i, j))
        if key not in mid:
            m = verts[i] + verts[j]
            verts.append(m / np.linalg.norm(m))
            mid[key] = len(verts) - 1
        return mid[key]
    tris = []
    for a, b, c in F:
        ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
        tris += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
    return np.asarray(verts, np.float32), np.asarray(tris, np.int32)


def quads_to_triangles(quads):
    """Each quad (p0, e1, e2; [n, 9] or flat) as the triangles (p0, p0 + e1,
    p0 + e1 + e2) and (p0, p0 + e1 + e2, p0 + e2) -- the quad's winding:
    (vertices [4 n, 3] float32, triangles [2 n, 3] int32)."""
    q = np.asarray(quads, np.float32).reshape(-1, 3, 3)
    p0, e1, e2 = q[:, 0], q[:, 1], q[:, 2]
    verts = np.stack([p0, p0 + e1, p0 + e1 + e2, p0 + e2], 1).reshape(-1, 3)
    base = 4 * np.arange(len(q), dtype=np.int32)[:, None]
    tris = np.concatenate([base + np.array([0, 1, 2], np.int32), base + np.array([0, 2, 3], np.int32)], 1)
    return verts.astype(np.float32), np.ascontiguousarray(tris.reshape(-1, 3), np.int32)


def _look_at(origin, target, up):
    """Mitsuba's lookAt as a row-major 4x4 camera-to-world (camera looks along +z)."""
    o, t, u = (np.asarray(x, np.float64) for x in (origin, target, up))
    z = (t - o) / np.linalg.norm(t - o)
    x = np.cross(u, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    M = np.eye(4)
    M[:3, 0], M[:3, 1], M[:3, 2], M[:3, 3] = x, y, z, o
    return M.reshape(-1).astype(np.float32)


def constant_environment(rgb):
    """The description fields of a `constant` environment emitter
    (emitters/constant.cpp): every ray that leaves the scene sees the radiance
    rgb."""
    return {"env_kind": 1, "env_radiance": np.asarray(rgb, np.float32).reshape(3)}


def latlong_direction(u, v):
    """The unit direction (emitter's local frame) of the lat-long texture
    coordinates (u, v) in [0, 1)^2 of a kind-2 environment -- the inverse of
    envmap.cpp:385-388's mapping u = atan2(x, -z) / 2 pi (mod 1), v = acos(y)
    / pi: row 0 of the map is the +y pole, u = 0 looks along -z."""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    phi, theta = 2.0 * np.pi * u, np.pi * v
    return np.stack([np.sin(theta) * np.sin(phi), np.cos(theta), -np.sin(theta) * np.cos(phi)], -1)


def sky_environment(width=256, height=128, sun_dir=(0.35, 0.8, 0.45), sun_radius_deg=4.0,
                    sun_radiance=(180.0, 165.0, 140.0), zenith=(0.25, 0.45, 0.9), horizon=(0.9, 0.9, 0.85),
                    to_world=None):
    """The description fields of a lat-long environment map holding a
    procedural sky: a zenith-to-horizon gradient (horizon colour below the
    horizon, dimmed to a third: the ground's bounce) plus a sun disc of
    sun_radius_deg about sun_dir with a smooth edge of a quarter of the radius.
    A stand-in for the Torus and Kitchen configurations' `sunsky` emitter, as
    the torus is for their geometry: Mitsuba's sun / sky model and its tables
    are not restated.  to_world: the emitter's 3x3 rotation (default the
    identity); the description carries its inverse."""
    uu, vv = np.meshgrid((np.arange(width) + 0.5) / width, (np.arange(height) + 0.5) / height)
    d = latlong_direction(uu, vv)                                     # [h, w, 3]
    up = np.clip(d[..., 1], 0.0, 1.0)[..., None]
    sky = np.asarray(horizon, np.float64) + (np.asarray(zenith, np.float64) - np.asarray(horizon, np.float64)) * up ** 0.5
    px = np.where(d[..., 1:2] >= 0.0, sky, np.asarray(horizon, np.float64) / 3.0)
    sun = np.asarray(sun_dir, np.float64)
    sun = sun / np.linalg.norm(sun)
    ang = np.degrees(np.arccos(np.clip(d @ sun, -1.0, 1.0)))
    disc = np.clip((sun_radius_deg * 1.25 - ang) / (0.25 * sun_radius_deg), 0.0, 1.0)[..., None]
    px = px + disc * np.asarray(sun_radiance, np.float64)
    R = np.eye(3) if to_world is None else np.asarray(to_world, np.float64).reshape(3, 3)
    return {"env_kind": 2, "env_pixels": np.ascontiguousarray(px, np.float32), "env_scale": 1.0,
            "env_world_to_local": np.linalg.inv(R).astype(np.float32).reshape(-1)}


def torus_scene(width=640, height=360, nu=96, nv=48, glass=True, environment=None, smooth=False,
                smooth_normals=False):
    """The Torus configuration's stand-in (test-suite/scenes/torus/torus.xml):
    a diffuse torus (reflectance .8, .8, .4; torus_mesh(nu, nv), R 1, r 0.4,
    lying on the floor) under a rough-dielectric case of quads (alpha 0.05,
    ior 1.5, the shipped dielectric_4c learned model) on a diffuse floor.  The
    reference lights the scene with `sunsky`.  environment: the env fields of
    the description (constant_environment / sky_environment) -- the scene is
    then open, the torus under its case on the floor under that sky, with no
    room and no lamp.  None (the default): a closed room of quads with a
    ceiling lamp, the proxy from before the device Li had an environment
    emitter.  The camera follows torus.xml's framing loosely: above and in
    front of the case, looking down at the torus.
    smooth: the materials torus.xml itself names -- the case a smooth
    dielectric (kind 5, ior 1.5: its `dielectric`, whose alpha attribute the
    plugin ignores; no learned model) and two metal pieces, an eighth of the
    ring each at opposite sides of it, smooth conductors
    (kind 6: its `conductor`) with a gray eta / k near aluminium's (1.2, 7.0);
    the reference's spectral .spd data of the metal is not used.  The rest of
    the torus stays diffuse.  False (the default): the scene as it was.
    smooth_normals: the torus carries its analytic vertex normals
    (mesh_normals): shaded, trained and guided as the curved surface it
    stands for.  False (the default): face normals, the scene as it was."""
    names = ["Room", "Floor", "Torus", "Glass", "Light"] + (["Metal"] if smooth else [])
    refl = {"Room": (0.6, 0.6, 0.6), "Floor": (0.5, 0.5, 0.5), "Torus": (0.8, 0.8, 0.4), "Glass": (1.0, 1.0, 1.0),
            "Light": (0.0, 0.0, 0.0), "Metal": (0.0, 0.0, 0.0)}
    quads, bsdf, emitter = [], [], []

    def box(lo, hi, name, inward, skip_bottom=False):
        lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
        M = np.zeros((3, 4))
        M[:, :3] = np.diag(0.5 * (hi - lo))
        M[:, 3] = 0.5 * (hi + lo)
        for k, (p0, e1, e2) in enumerate(_cube_faces(M)):
            if skip_bottom and k == 3:      # the face y = lo (ax 1, s -1)
                continue
            quads.append(np.concatenate((p0, e2, e1) if inward else (p0, e1, e2)))
            bsdf.append(names.index(name)); emitter.append(-1)
    if environment is None:
        box((-4.0, 0.0, -4.0), (4.0, 5.0, 4.0), "Room", inward=True, skip_bottom=True)
    quads.append(np.array([-4.0, 0.0, -4.0, 0.0, 0.0, 8.0, 8.0, 0.0, 0.0]))      # floor, normal +y
    bsdf.append(names.index("Floor")); emitter.append(-1)
    if environment is None:
        quads.append(np.array([-1.5, 4.99, -1.5, 3.0, 0.0, 0.0, 0.0, 0.0, 3.0]))     # lamp, normal -y
        bsdf.append(names.index("Light")); emitter.append(0)
    else:
        extra_env = dict(environment)
    bp = np.zeros((len(names), 8), np.float32)
    extra = {}
    if glass:
        # the case stands 0.02 above the floor: its bottom face is not coplanar with it
        box((-1.7, 0.02, -1.7), (1.7, 1.2, 1.7), "Glass", inward=False)
        if smooth:
            bp[names.index("Glass")], refl["Glass"] = smooth_dielectric_params(int_ior=1.5, ext_ior=1.0)
        else:
            bp[names.index("Glass")], refl["Glass"] = dielectric_params(int_ior=1.5, ext_ior=1.0, alpha=0.05)
            model = load_learned_nd(LEARNED_DIELECTRIC)
            extra["learned_models_nd"] = [model if nm == "Glass" else None for nm in names]
    T = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0.45], [0, 0, 1.0, 0]])
    verts, tris, vnrm = torus_mesh(nu, nv, 1.0, 0.4, to_world=T, normals=True)
    if smooth_normals:
        extra["mesh_normals"] = vnrm.reshape(-1)
    tri_bsdf = np.full(len(tris), names.index("Torus"), np.int32)
    if smooth:
        # torus_mesh orders its triangles by the ring index: two opposite arcs of an eighth of the ring each
        bp[names.index("Metal")] = smooth_conductor_params()
        ring = np.arange(len(tris)) // (2 * nv)
        tri_bsdf[((ring % (nu // 2)) < max(1, nu // 8))] = names.index("Metal")
    if environment is not None:
        extra.update(extra_env)
    return {**extra,
        "quads": np.asarray(quads, np.float32).reshape(-1),
        "bsdf": np.asarray(bsdf, np.int32),
        "bsdf_params": bp.reshape(-1),
        "reflectance": np.asarray([refl[n] for n in names], np.float32).reshape(-1),
        "emitter": np.asarray(emitter, np.int32),
        "radiance": np.asarray([12.0, 12.0, 12.0], np.float32),
        "mesh_vertices": verts.reshape(-1),
        "triangles": tris.reshape(-1),
        "tri_bsdf": tri_bsdf,
        "camera_to_world": _look_at((0.0, 3.2, 3.6), (0.0, 0.4, 0.0), (0.0, 1.0, 0.0)),
        "fov_x_deg": 45.0,
        "near_clip": 1e-2,
        "width": width,
        "height": height,
    }


def sheet_mesh(nx, nz, x=(-1.8, 1.8), z=(1.4, -2.6), y0=1.6, amplitude=0.45, waves=1.25, phase=np.pi,
               normals=False, uvs=False):
    """An open sheet: the height field y = y0 + amplitude sin(2 pi waves s +
    phase) over x[0]..x[1] and, along s in [0, 1], z[0]..z[1], as nx x nz
    cells of two triangles with the face normals on the +y side: (vertices
    [(nx + 1)(nz + 1), 3] float32, triangles [2 nx nz, 3] int32).  normals:
    also the height field's analytic unit normals at the vertices, on the +y
    side (float32, third of the tuple).  uvs: also the vertices' texture
    coordinates (a, s), both over [0, 1] (float32 [., 2], last of the tuple)."""
    a = np.linspace(0.0, 1.0, nx + 1)
    s = np.linspace(0.0, 1.0, nz + 1)
    aa, ss = np.meshgrid(a, s, indexing="ij")
    P = np.stack([x[0] + (x[1] - x[0]) * aa, y0 + amplitude * np.sin(2.0 * np.pi * waves * ss + phase),
                  z[0] + (z[1] - z[0]) * ss], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nx), np.arange(nz), indexing="ij")
    p00 = (i * (nz + 1) + j).reshape(-1)
    p10, p01, p11 = p00 + (nz + 1), p00 + 1, p00 + (nz + 1) + 1
    tris = np.concatenate([np.stack([p00, p10, p11], -1), np.stack([p00, p11, p01], -1)], 1).reshape(-1, 3)
    # (dP/da) x (dP/ds) points along +y when x grows with a and z falls with s
    if (x[1] - x[0]) * (z[1] - z[0]) > 0:
        tris = tris[:, ::-1]
    if normals:
        # y = f(s), z = z0 + (z1 - z0) s: the normal is (0, 1, -dy/dz) normalised
        dyds = amplitude * 2.0 * np.pi * waves * np.cos(2.0 * np.pi * waves * ss + phase)
        Nn = np.stack([np.zeros_like(ss), np.ones_like(ss), -dyds / (z[1] - z[0])], -1).reshape(-1, 3)
        Nn /= np.linalg.norm(Nn, axis=1, keepdims=True)
    out = (P.astype(np.float32), np.ascontiguousarray(tris, np.int32))
    if normals:
        out += (Nn.astype(np.float32),)
    if uvs:
        out += (np.stack([aa, ss], -1).reshape(-1, 2).astype(np.float32),)
    return out


SHEET_MATERIALS = ("diffuse", "plastic", "conductor", "phong", "mirror")   # kinds 0, 1, 2, 3, 6


def sheet_scene(width=640, height=360, nx=16, nz=48, material="diffuse", twosided=True, environment=None,
                reflectance=(0.7, 0.6, 0.4), learned=True, patch=False, smooth_normals=False, texture=None):
    """An open surface for the `twosided` adapter: torus_scene's lit room (or,
    with environment=, its open floor under that sky) holding a sheet --
    sheet_mesh(nx, nz), a sine wave hanging at the camera's height and running
    away from it, so the camera looks under its near edge at the back of the
    first slope and over that edge at the front of the slopes behind it.
    Every face normal is on the sheet's upper side: the lamp lights the front,
    the floor's bounce the back.  material: one of SHEET_MATERIALS (kinds 0,
    1, 2, 3 and 6) over `reflectance`, parametrised as cornell_box's plastic /
    conductor / phong / mirror; learned: a conductor or Phong sheet carries
    the shipped learned model.  twosided: the sheet's BSDF is under the
    adapter (the default; False: the one-sided BSDF, black from behind).
    patch: a two-sided rough-conductor quad (alpha 0.2, its learned SDMM4)
    lying face up above the sheet and the camera: what reaches it from below
    meets its back, and in the open scene (environment=) nothing lies above
    it, so every hit on it is one from behind.  smooth_normals: the sheet
    carries its analytic vertex normals (mesh_normals).  texture: a texture
    (checker_texture / ramp_texture) on the sheet's reflectance, looked up at
    the sheet's own uvs (mesh_uvs) -- a diffuse, plastic or Phong sheet, whose
    sampling weight then comes from the texture's mean."""
    if material not in SHEET_MATERIALS:
        raise ValueError(f"material: one of {SHEET_MATERIALS}")
    if texture is not None:
        if material not in ("diffuse", "plastic", "phong"):
            raise ValueError("texture: on a diffuse, plastic or phong sheet")
        reflectance = tuple(float(c) for c in texture_mean(texture))
    names = ["Room", "Floor", "Sheet", "Light"] + (["Patch"] if patch else [])
    refl = {"Room": (0.6, 0.6, 0.6), "Floor": (0.5, 0.5, 0.5), "Sheet": tuple(reflectance), "Light": (0.0, 0.0, 0.0),
            "Patch": (0.0, 0.0, 0.0)}
    quads, bsdf, emitter = [], [], []
    if environment is None:
        M = np.zeros((3, 4))
        M[:, :3] = np.diag([4.0, 2.5, 4.0])
        M[:, 3] = (0.0, 2.5, 0.0)
        for k, (p0, e1, e2) in enumerate(_cube_faces(M)):
            if k == 3:                          # the face y = 0: the floor below
                continue
            quads.append(np.concatenate((p0, e2, e1)))     # inward
            bsdf.append(names.index("Room")); emitter.append(-1)
    quads.append(np.array([-4.0, 0.0, -4.0, 0.0, 0.0, 8.0, 8.0, 0.0, 0.0]))      # floor, normal +y
    bsdf.append(names.index("Floor")); emitter.append(-1)
    if environment is None:
        quads.append(np.array([-1.5, 4.99, -1.5, 3.0, 0.0, 0.0, 0.0, 0.0, 3.0]))     # lamp, normal -y
        bsdf.append(names.index("Light")); emitter.append(0)
    if patch:
        quads.append(np.array([-3.6, 3.2, -3.6, 0.0, 0.0, 2.4, 2.4, 0.0, 0.0]))     # normal +y: seen from below
        bsdf.append(names.index("Patch")); emitter.append(-1)
    bp = np.zeros((len(names), 8), np.float32)
    b = names.index("Sheet")
    extra = {}
    tint = tuple(min(1.0, 1.25 * c) for c in reflectance)
    models = [None] * len(names)
    if material == "plastic":
        bp[b] = plastic_params(reflectance)
    elif material == "conductor":
        bp[b] = conductor_params(tint)
        if learned:
            models[b] = load_learned(LEARNED_CONDUCTOR)
    elif material == "phong":
        bp[b], refl["Sheet"] = phong_params(reflectance, (0.4, 0.4, 0.4), 30.0)
        if learned:
            extra["learned_models_nd"] = [load_learned_nd(LEARNED_PHONG) if nm == "Sheet" else None for nm in names]
    elif material == "mirror":
        bp[b] = smooth_conductor_params(tint)
    if patch:
        bp[names.index("Patch")] = conductor_params((0.9, 0.9, 0.9))
        models[names.index("Patch")] = load_learned(LEARNED_CONDUCTOR)
    if any(m is not None for m in models):
        extra["learned_models"] = models
    if twosided:
        extra["bsdf_twosided"] = np.asarray([int(nm in ("Sheet", "Patch")) for nm in names], np.int32)
    if environment is not None:
        extra.update(environment)
    verts, tris, vnrm, vuv = sheet_mesh(nx, nz, normals=True, uvs=True)
    if smooth_normals:
        extra["mesh_normals"] = vnrm.reshape(-1)
    if texture is not None:
        extra["mesh_uvs"] = vuv.reshape(-1)
        extra["textures"] = [texture]
        extra["bsdf_texture"] = np.asarray([0 if nm == "Sheet" else -1 for nm in names], np.int32)
    return {**extra,
        "quads": np.asarray(quads, np.float32).reshape(-1),
        "bsdf": np.asarray(bsdf, np.int32),
        "bsdf_params": bp.reshape(-1),
        "reflectance": np.asarray([refl[n] for n in names], np.float32).reshape(-1),
        "emitter": np.asarray(emitter, np.int32),
        "radiance": np.asarray([12.0, 12.0, 12.0], np.float32),
        "mesh_vertices": verts.reshape(-1),
        "triangles": tris.reshape(-1),
        "tri_bsdf": np.full(len(tris), b, np.int32),
        "camera_to_world": _look_at((0.0, 1.75, 3.9), (0.0, 1.5, 0.0), (0.0, 1.0, 0.0)),
        "fov_x_deg": 45.0,
        "near_clip": 1e-2,
        "width": width,
        "height": height,
    }


def mirror_z(desc, keep=()):
    """The description's mirror image in the plane z = 0: every z coordinate
    negated (quad corners and edges, mesh vertices, the camera's position and
    the z row of its axes), flip_normals toggled on every quad and triangle
    except those listed in `keep` (quad ids; a triangle is n_quads + its
    index) -- the mirror reverses a primitive's winding, so toggling keeps its
    normal the mirrored one, and a kept primitive keeps the normal it had: it
    is then met from the other side.  Order and every other field are the
    same; the environment's transform is not mirrored.
    With mesh_normals their z is negated too, and the triangles' rule turns
    round: the flag does not undo a winding there, it negates the shading
    normal ns itself (the winding's face normal only follows ns), so a
    triangle's flag is left as it is -- ns is then the mirrored one, and ng,
    whose unflipped face normal the mirror negated, is turned back onto it --
    and a triangle listed in `keep` gets its flag toggled: ns = -mirror(ns),
    met from the other side.  (Where the interpolated normal vanishes the
    library falls back to the face normal with the flag applied, which this
    rule leaves negated.)  mesh_uvs, textures and bsdf_texture are carried as
    they are: a quad's (a, b) and a triangle's (u, v) are the mirrored
    primitive's bit for bit (a zero may change its sign).  Mirroring twice gives the description back."""
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in desc.items()}
    keep = set(int(k) for k in keep)
    nq = 0
    if "quads" in desc and np.asarray(desc["quads"]).size:
        q = np.array(desc["quads"], np.float32).reshape(-1, 3, 3)
        q[:, :, 2] = -q[:, :, 2]
        nq = len(q)
        out["quads"] = q.reshape(-1)
        fl = np.array(desc.get("flip_normals", np.zeros(nq, np.int32)), np.int32)
        out["flip_normals"] = np.asarray([f if i in keep else 1 - f for i, f in enumerate(fl)], np.int32)
    if "mesh_vertices" in desc:
        v = np.array(desc["mesh_vertices"], np.float32).reshape(-1, 3)
        v[:, 2] = -v[:, 2]
        out["mesh_vertices"] = v.reshape(-1)
        nt = np.asarray(desc["triangles"]).size // 3
        fl = np.array(desc["tri_flip_normals"], np.int32) if desc.get("tri_flip_normals") is not None \
            else np.zeros(nt, np.int32)
        if desc.get("mesh_normals") is not None:
            n = np.array(desc["mesh_normals"], np.float32).reshape(-1, 3)
            n[:, 2] = -n[:, 2]
            out["mesh_normals"] = n.reshape(-1)
            out["tri_flip_normals"] = np.asarray([1 - f if nq + i in keep else f for i, f in enumerate(fl)], np.int32)
        else:
            out["tri_flip_normals"] = np.asarray([f if nq + i in keep else 1 - f for i, f in enumerate(fl)],
                                                 np.int32)
    cam = np.array(desc["camera_to_world"], np.float32).reshape(4, 4)
    cam[2, :] = -cam[2, :]
    out["camera_to_world"] = cam.reshape(-1)
    return out


def diffuse_learned_bsdf(n_bsdfs: int, sigma: float = 0.65):
    """Learned-BSDF tables for diffuse materials (the plugin's sampleProduct
    path; the suite's `diffuse.sdmm` files are LFS pointers, so the table is
    synthesised): per BSDF ONE directional lobe -- the plugin's diffuse case
    re-centres only slice 0 on the shading normal (sdmm_proc.cpp:335-339), so
    a diffuse learned BSDF is one lobe around the normal.  sigma: the lobe's
    tangent-space standard deviation (0.65 rad ~ the spread of a cosine lobe).
    Returns (weights (B, 1), local means (B, 1, 3), covs (B, 1, 4), diffuse (B,))."""
    B = int(n_bsdfs)
    w = np.ones((B, 1), np.float32)
    m = np.zeros((B, 1, 3), np.float32)
    m[..., 2] = 1.0
    cov = np.zeros((B, 1, 4), np.float32)
    cov[..., 0] = cov[..., 3] = sigma * sigma
    return w, m, cov, np.ones(B, np.uint8)
