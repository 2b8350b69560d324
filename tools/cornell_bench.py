"""The Cornell Box line of bench.py alone (configs[0] on the device).

--glossy NAME ...  those BSDFs as rough conductors (bench.py's
                   cornell_k512_glossy_product line: --glossy TallBox Floor
                   --product --K 512 --modes 0)
--phong NAME ...   those BSDFs as Phong with the learned SDMM5 instead
--dielectric NAME ...  those BSDFs as rough dielectrics (glass) with the
                   learned SDMM5, a cube lifted off the floor by 0.02
--repeat N         N timed lines per configuration (A/B runs: medians, spreads)
"""
import functools
import importlib
import importlib.util
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
spec = importlib.util.spec_from_file_location("bench", ROOT / "bench.py")
bench = importlib.util.module_from_spec(spec)
spec.loader.exec_module(bench)

if __name__ == "__main__":
    import torch
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, nargs="+", default=[16])
    ap.add_argument("--modes", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--product", action="store_true", help="sampleProduct (the learned diffuse lobes)")
    ap.add_argument("--glossy", nargs="*", default=[], help="BSDFs rendered as rough conductors")
    ap.add_argument("--phong", nargs="*", default=[], help="BSDFs rendered as Phong (learned SDMM5)")
    ap.add_argument("--dielectric", nargs="*", default=[], help="BSDFs rendered as rough dielectrics (learned SDMM5)")
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--summary", action="store_true", help="one line per run, no per-iteration lines")
    a = ap.parse_args()
    pkg = bench.load_pkg()
    if a.phong:
        # bench.cornell_bench builds its scene with scenes.cornell_box(w, h, conductor=glossy)
        scenes = importlib.import_module("sdmm_mitsuba_amd.scenes")
        scenes.cornell_box = functools.partial(scenes.cornell_box, phong=tuple(a.phong))
    if a.dielectric:
        scenes = importlib.import_module("sdmm_mitsuba_amd.scenes")
        scenes.cornell_box = functools.partial(scenes.cornell_box, dielectric=tuple(a.dielectric),
                                               dielectric_lift=0.02)
    for K in a.K:
      for mode in a.modes:
        for _ in range(a.repeat):
            out = bench.cornell_bench(pkg, torch.device("cuda", 0), None, 1, optimize_async=mode, K=K,
                                      product=a.product, glossy=tuple(a.glossy))
            if a.phong:
                out["workload"] += " (Phong " + "/".join(a.phong) + ")"
            if a.dielectric:
                out["workload"] += " (rough dielectric " + "/".join(a.dielectric) + ")"
            print(json.dumps({k: v for k, v in out.items() if k != "iterations"}), flush=True)
            if not a.summary:
                for it in out["iterations"]:
                    print(json.dumps(it), flush=True)
