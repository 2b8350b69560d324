"""bench.py as a command: a plain run prints the headline line only, --steps
sets the number of timed launches, and --dump-outputs writes the
responsibilities the timed path computed (here N is below the row-sample cap,
so every row is kept) -- bitwise what the same seeded workload gives in this
process."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]


def test_plain_run_line_and_dump(pkg, synth, gpu, tmp_path):
    import torch
    N, K, warm = 5000, 128, 2          # N: no multiple of the kernels' tiles
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--settle", "0", "--N", str(N), "--em-warm", str(warm), "--dump-outputs",
                        str(tmp_path / "out")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["settle_launches"] == 0
    assert out["unit"] == "samples/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(N / (out["ms_per_step"] * 1e-3), rel=1e-9)
    # the lines behind --full are not measured by a plain run
    for key in ("em_step", "estep_stats", "guide", "leaf_em", "stree", "cornell", "large_k", "cpu_baseline"):
        assert key not in out
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["resp.npy"]
    got = np.load(tmp_path / "out" / "resp.npy")
    assert got.dtype == np.float32 and got.shape == (N, K)

    b = synth.em_batch(N, 128)
    pos, nrm = synth.model_seed_points(b, K)
    mix = pkg.SDMM(K)
    mix.init_hemisphere(pos, nrm, synth.DEPTH_PRIOR, synth.SPATIAL_DISTANCE, synth.SEED_MODEL)
    ds = pkg.DeviceSamples.from_numpy(b["x"], b["w"], b["hpdf"], b["is_diffuse"], device=gpu)
    for _ in range(warm):
        mix.optimize(ds)
    resp = torch.empty((N, K), device=gpu)
    mix.posterior(ds, resp)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got, resp.cpu().numpy())
