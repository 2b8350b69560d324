"""The Cornell Box line of bench.py alone (configs[0] on the device).

--glossy NAME ...  those BSDFs as rough conductors (bench.py's
                   cornell_k512_glossy_product line: --glossy TallBox Floor
                   --product --K 512 --modes 0)
--phong NAME ...   those BSDFs as Phong with the learned SDMM5 instead
--dielectric NAME ...  those BSDFs as rough dielectrics (glass) with the
                   learned SDMM5, a cube lifted off the floor by 0.02
--torus            the torus scene instead (scenes.torus_scene: a triangle mesh
                   under a glass case; --tess NUxNV its tessellation, default
                   96x48) through the same loop; SDMM_MESH_BRUTE=1 in the
                   environment makes the Li kernels loop over all triangles
                   instead of walking the BVH (A/B)
--env              with --torus: the open scene -- no room, no lamp, the torus
                   under its case on the floor under scenes.sky_environment()
                   (a lat-long environment map)
--smooth-normals   with --torus: the torus carries its analytic vertex normals
                   (scenes.torus_scene(smooth_normals=True)): the Li kernels'
                   NRM variants run
--textured         the Cornell box with scenes.cornell_box(textured=True): a
                   checker on the floor, a ramp on a Phong back wall -- the Li
                   kernels' TEX variants run (not with --torus)
--env-eval N       time sdmm_env_eval on 2^N random directions against a
                   1024x512 map (device time per launch from events); with
                   --repeat 0 nothing else runs
--intersect N      with --torus: also time sdmm_scene_intersect on 2^N
                   camera-like rays against the scene without its case, BVH
                   and brute force (rays/s), and a plain unguided 8-spp pass;
                   --repeat 0 then skips the training loop
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
    ap.add_argument("--torus", action="store_true", help="the torus scene (triangle mesh) instead of the Cornell box")
    ap.add_argument("--tess", default="96x48", help="--torus: tessellation NUxNV")
    ap.add_argument("--intersect", type=int, default=0, help="--torus: time Scene.intersect on 2^N rays")
    ap.add_argument("--env", action="store_true", help="--torus: the open scene under a sky environment map")
    ap.add_argument("--smooth-normals", action="store_true", help="--torus: vertex normals on the torus")
    ap.add_argument("--textured", action="store_true", help="bitmap textures on the floor and the back wall")
    ap.add_argument("--env-eval", type=int, default=0, help="time Scene.env_eval on 2^N directions, 1024x512 map")
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
    if a.textured:
        if a.torus or "Floor" in a.glossy + a.phong + a.dielectric or "BackWall" in a.glossy + a.phong + a.dielectric:
            ap.error("--textured: the Cornell box, Floor and BackWall taking no other material")
        scenes = importlib.import_module("sdmm_mitsuba_amd.scenes")
        scenes.cornell_box = functools.partial(scenes.cornell_box, textured=True)
    if a.env and not a.torus:
        ap.error("--env goes with --torus")
    if a.smooth_normals and not a.torus:
        ap.error("--smooth-normals goes with --torus")
    if a.env_eval:
        import numpy as np
        scenes = importlib.import_module("sdmm_mitsuba_amd.scenes")
        dev = torch.device("cuda", 0)
        sc = pkg.Scene(scenes.torus_scene(64, 36, 24, 12, environment=scenes.sky_environment(1024, 512)))
        n = 1 << a.env_eval
        g = torch.Generator(device=dev).manual_seed(1)
        dirs = torch.randn(n, 3, device=dev, generator=g)
        dirs = dirs / dirs.norm(dim=1, keepdim=True)
        d = [dirs[:, i].contiguous() for i in range(3)]
        launches = 20
        sc.env_eval(d)
        torch.cuda.synchronize()
        times = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                rgb = sc.env_eval(d)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) / launches)
        print(json.dumps({"env_eval": "1024x512", "directions": n, "launches_per_group": launches,
                          "ms": [round(t, 4) for t in times], "directions_per_s": n / (min(times) * 1e-3),
                          "mean_radiance": float(torch.stack(rgb).mean())}), flush=True)
    if a.torus:
        import os
        import time
        scenes = importlib.import_module("sdmm_mitsuba_amd.scenes")
        nu, nv = (int(x) for x in a.tess.lower().split("x"))
        sky = scenes.sky_environment() if a.env else None
        # (smooth_normals is passed only when asked for: without the flag the call is what it always was)
        nkw = {"smooth_normals": True} if a.smooth_normals else {}
        scenes.cornell_box = lambda w, h, **kw: (scenes.torus_scene(w, h, nu, nv, environment=sky, **nkw) if a.env
                                                 else scenes.torus_scene(w, h, nu, nv, **nkw))
        brute = os.environ.get("SDMM_MESH_BRUTE") == "1"
        if a.intersect:
            dev = torch.device("cuda", 0)
            # (without the glass case: every ray would stop at it, and the walk would have nothing to do)
            sc = pkg.Scene(scenes.torus_scene(640, 360, nu, nv, glass=False))
            n = 1 << a.intersect
            g = torch.Generator(device=dev).manual_seed(1)
            # camera-like: one origin, directions in a cone about the view axis
            cam = torch.tensor([0.0, 3.2, 3.6], device=dev)
            axis = torch.tensor([0.0, -2.8, -3.6], device=dev)
            dirs = axis / axis.norm() + 0.5 * (torch.rand(n, 3, device=dev, generator=g) - 0.5)
            dirs = dirs / dirs.norm(dim=1, keepdim=True)
            o = [cam[i].expand(n).contiguous() for i in range(3)]
            d = [dirs[:, i].contiguous() for i in range(3)]
            # device time by events over several back-to-back launches (the
            # call also allocates its two output planes from torch's cache),
            # three such groups, the best one reported
            for mode in (0, 1):
                launches = 3 if mode else 20
                sc.intersect(o, d, 1e-2, float("inf"), mode)
                torch.cuda.synchronize()
                times = []
                for _ in range(3):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(launches):
                        prim, _ = sc.intersect(o, d, 1e-2, float("inf"), mode)
                    e1.record()
                    torch.cuda.synchronize()
                    times.append(e0.elapsed_time(e1) / launches)
                print(json.dumps({"intersect": "brute" if mode else "bvh", "triangles": 2 * nu * nv, "rays": n,
                                  "launches_per_group": launches, "ms": [round(t, 4) for t in times],
                                  "rays_per_s": n / (min(times) * 1e-3),
                                  "mesh_hits": int((prim >= sc.n_quads).sum())}), flush=True)
            # a plain unguided pass (8 spp, no training) of the scene with its case (--env: the open scene)
            sc = pkg.Scene(scenes.cornell_box(640, 360))
            _, _, tmin, tmax = sc.normalization()
            tree = pkg.STree(tmin, tmax)
            tree.split_to_depth(2)
            times = []
            for i in range(4):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                sc.render(tree, None, spp=8, guided=False, seed=1 + i)
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
            print(json.dumps({"unguided_pass_ms": [round(t * 1e3, 3) for t in times[1:]], "triangles": 2 * nu * nv,
                              "mesh": "brute" if brute else "bvh", "env": bool(a.env)}), flush=True)
    for K in a.K:
      for mode in a.modes:
        for _ in range(a.repeat):
            out = bench.cornell_bench(pkg, torch.device("cuda", 0), None, 1, optimize_async=mode, K=K,
                                      product=a.product, glossy=tuple(a.glossy))
            if a.torus:
                out["workload"] = out["workload"].replace("Cornell Box", f"Torus scene ({a.tess}, " +
                                                          ("brute force" if brute else "BVH") +
                                                          (", open under a sky map" if a.env else "") +
                                                          (", vertex normals" if a.smooth_normals else "") + ")")
                its = out["iterations"]
                out["first_pass_ms"] = round(its[0]["ms"], 3)     # unguided render + push + optimize
                out["guided_pass_ms"] = [round(x["ms"], 3) for x in its if not x["train"]]
            if a.phong:
                out["workload"] += " (Phong " + "/".join(a.phong) + ")"
            if a.dielectric:
                out["workload"] += " (rough dielectric " + "/".join(a.dielectric) + ")"
            if a.textured:
                out["workload"] += " (textured floor and back wall)"
            print(json.dumps({k: v for k, v in out.items() if k != "iterations"}), flush=True)
            if not a.summary:
                for it in out["iterations"]:
                    print(json.dumps(it), flush=True)
