#!/usr/bin/env python3
"""Write the synthetic learned Phong BSDF the Phong Cornell scene uses
(sdmm-mitsuba_amd/data/phong_4c.sdmm5.json).

The reference conditions each Phong material's learned SDMM5 (BSDF::SDMM5,
include/mitsuba/render/bsdf.h:316-324: (theta_i, specWeight, log exponent) x
direction) per bounce, pruned to 2 with component 1 -- the diffuse lobe --
always kept (phong.cpp:75-90); its file (phong_4c.sdmm) is a Git-LFS pointer
in the snapshot, so a synthetic 4-component model with the same structure
stands in, built like tools/make_learned_conductor.py's as a joint Gaussian
per component rather than fitted:
  * component 1, the diffuse lobe: a broad lobe about the normal (tangent
    standard deviation 0.65 rad, the spread of a cosine lobe), broad in the
    condition, S_dc = 0 (it does not move with the condition);
  * components 0, 2, 3, the specular lobes: at the mirror direction of an
    incident direction at elevation theta_k (azimuth 0, the canonical frame of
    getDMM), on a theta x log-exponent grid; the tangent coordinates follow
    theta as t = v (theta - theta_k) + n with v the mirror direction's
    derivative, n an isotropic lobe of standard deviation 1 / sqrt(e_k + 1)
    (a cos^e lobe's spread).
So every joint covariance is PD by construction.

    python tools/make_learned_phong.py [out.json]
"""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))
from make_learned_conductor import coordinates  # noqa: E402

OUT = ROOT / "sdmm-mitsuba_amd" / "data" / "phong_4c.sdmm5.json"


def model():
    s_theta, s_spec, s_lexp = 0.35, 0.4, 1.2
    w, means, covs = [], [], []

    def specular(th, exponent):
        mu = np.array([-np.sin(th), 0.0, np.cos(th)])
        mu = (mu / np.linalg.norm(mu)).astype(np.float32)
        T = coordinates(mu).astype(np.float64)
        v = T[:2] @ np.array([-np.cos(th), 0.0, -np.sin(th)])     # d(mirror direction) / d(theta)
        # x = (theta, specWeight, log exponent, t1, t2) = A z, z ~ N(0, I)
        A = np.zeros((5, 5))
        A[0, 0], A[1, 1], A[2, 2] = s_theta, s_spec, s_lexp
        A[3:, 0] = v * s_theta
        A[3, 3] = A[4, 4] = 1.0 / np.sqrt(exponent + 1.0)
        w.append(0.2)
        means.append([th, 0.6, np.log(exponent), *mu.tolist()])
        covs.append((A @ A.T).reshape(-1).tolist())

    specular(0.35, 20.0)
    # the diffuse lobe (index 1: phong.cpp:76)
    w.append(0.4)
    means.append([0.7, 0.4, np.log(30.0), 0.0, 0.0, 1.0])
    covs.append(np.diag([0.8, 0.5, 2.0, 0.65, 0.65]) ** 2)
    covs[-1] = covs[-1].reshape(-1).tolist()
    specular(1.05, 20.0)
    specular(0.7, 300.0)
    return np.float32(w), np.float32(means), np.float32(covs)


def main():
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else OUT
    w, mu, cv = model()
    f9 = lambda a: [float(f"{float(x):.9g}") for x in np.asarray(a, np.float32).reshape(-1)]
    doc = {"format": "sdmm-amd.sdmm5", "version": 1, "C": 3, "M": int(len(w)), "weights": f9(w), "means": f9(mu),
           "covs": f9(cv)}
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(doc) + "\n")
    print(out)


if __name__ == "__main__":
    main()
