#!/usr/bin/env python3
"""optimize (one EM step) followed by one posterior at N = 131072, K = 128:
device time per pair from one event pair around 100 pairs, five times; and the
same for optimize alone and posterior alone."""
import importlib, json, statistics, sys
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import torch
from conftest import load_pkg
pkg = load_pkg()
synth = importlib.import_module("sdmm_mitsuba_amd.synth")
dev = torch.device("cuda:0")
K, N = 128, 131072
b = synth.em_batch(N, 128)
pos, nrm = synth.model_seed_points(b, K)
mix = pkg.SDMM(K)
mix.init_hemisphere(pos, nrm, synth.DEPTH_PRIOR, synth.SPATIAL_DISTANCE, synth.SEED_MODEL)
ds = pkg.DeviceSamples.from_numpy(b["x"], b["w"], b["hpdf"], b["is_diffuse"], device=dev)
resp = torch.empty((N, K), device=dev)
def pair():
    mix.optimize(ds); mix.posterior(ds, resp)
def opt():
    mix.optimize(ds)
def post():
    mix.posterior(ds, resp)
def timed(fn, reps=100):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps
for _ in range(300): pair()
out = {}
for name, fn in (("pair", pair), ("optimize", opt), ("posterior", post), ("pair2", pair)):
    ts = [timed(fn) for _ in range(5)]
    out[name + "_us"] = [round(t, 2) for t in ts]
    out[name + "_median_us"] = round(statistics.median(ts), 2)
out["kernel"] = mix.kernel_name("resp")
out["builds"] = mix.layout().get("resp_image_builds")
print(json.dumps(out))
