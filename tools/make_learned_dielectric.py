#!/usr/bin/env python3
"""Write the synthetic learned rough-dielectric BSDF the glass Cornell scene
uses (sdmm-mitsuba_amd/data/dielectric_4c.sdmm5.json).

The reference conditions each rough dielectric's learned SDMM5 (BSDF::SDMM5,
include/mitsuba/render/bsdf.h:316-324: (theta_i, alpha, eta) x direction) per
bounce, pruned to 2 with no forced lobe (roughdielectric.cpp:198-211); its
file (dielectric_4c.sdmm) is a Git-LFS pointer in the snapshot, so a synthetic
4-component model with the same structure stands in, built like
tools/make_learned_conductor.py's as a joint Gaussian per component rather
than fitted.  The components sit on a two-point grid (theta_k, alpha_k); at
each point
  * a reflected lobe at the mirror direction of an incident direction at
    elevation theta_k (azimuth 0, the canonical frame of getDMM), tangent
    standard deviation 2 alpha_k (a Beckmann lobe's reflected spread);
  * a transmitted lobe at the direction refracted by ETA, below the surface,
    tangent standard deviation alpha_k (refraction bends the microfacet
    normal's deviation by about (eta - 1) / eta of what reflection's 2 does),
    four times as heavy: most of the energy goes through.
The tangent coordinates follow theta as t = v (theta - theta_k) + n with v the
lobe direction's derivative in theta, so S_dc is non-zero (the conditional mean
follows theta_i), every joint covariance is PD by construction, and the
tangent spread grows with alpha along the grid.

    python tools/make_learned_dielectric.py [out.json]

The file is written by the library (sdmm_learned_save_json), so this needs the
built package.
"""
import importlib.util
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))
from make_learned_conductor import coordinates  # noqa: E402

OUT = ROOT / "sdmm-mitsuba_amd" / "data" / "dielectric_4c.sdmm5.json"
ETA = 1.5046 / 1.000277      # bk7 / air, the plugin's defaults


def model():
    grid = ((0.35, 0.1), (1.05, 0.35))
    s_theta, s_alpha, s_eta = 0.35, 0.12, 0.3
    w, means, covs = [], [], []

    def lobe(th, al, mu, dmu, weight, spread):
        mu = (mu / np.linalg.norm(mu)).astype(np.float32)
        T = coordinates(mu).astype(np.float64)
        v = T[:2] @ dmu
        # x = (theta, alpha, eta, t1, t2) = A z, z ~ N(0, I)
        A = np.zeros((5, 5))
        A[0, 0], A[1, 1], A[2, 2] = s_theta, s_alpha, s_eta
        A[3:, 0] = v * s_theta
        A[3, 3] = A[4, 4] = spread
        w.append(weight)
        means.append([th, al, ETA, *mu.tolist()])
        covs.append((A @ A.T).reshape(-1).tolist())

    for th, al in grid:
        # the mirror direction and its derivative in theta
        lobe(th, al, np.array([-np.sin(th), 0.0, np.cos(th)]), np.array([-np.cos(th), 0.0, -np.sin(th)]), 0.1,
             2.0 * al)
        # the refracted direction -(sin theta / eta, 0, cos theta_t)
        st = np.sin(th) / ETA
        ct = np.sqrt(1.0 - st * st)
        dst = np.cos(th) / ETA
        lobe(th, al, np.array([-st, 0.0, -ct]), np.array([-dst, 0.0, st * dst / ct]), 0.4, al)
    return np.float32(w), np.float32(means), np.float32(covs)


def main():
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else OUT
    pkg_dir = ROOT / "sdmm-mitsuba_amd"
    spec = importlib.util.spec_from_file_location("sdmm_mitsuba_amd", pkg_dir / "__init__.py",
                                                  submodule_search_locations=[str(pkg_dir)])
    pkg = importlib.util.module_from_spec(spec)
    sys.modules["sdmm_mitsuba_amd"] = pkg
    spec.loader.exec_module(pkg)
    w, mu, cv = model()
    out.parent.mkdir(parents=True, exist_ok=True)
    pkg.LearnedBSDFND(w, mu, cv, 3).save_json(out)
    print(out)


if __name__ == "__main__":
    main()
