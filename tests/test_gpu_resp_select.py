"""The E-step kernel choice per K and environment, through the public API.

sdmm_create picks the responsibility kernel from K, SDMM_RESP_KERNEL and
SDMM_RESP_IMAGE, and the statistics kernel from K.  Each row below creates an
uninitialised mixture and asserts the exact kernel names and layouts the
handle reports; no kernel is launched.  bench.py compares these names with
recorded ones, so they are part of the library's contract.
"""
import pytest

pytestmark = pytest.mark.gpu

# (SDMM_RESP_KERNEL, K, name("resp"), layout resp, split kernel?)
ROWS = [
    (None, 128, "estep_resp_split_band_kernel<8,4,3>", (2, 64), True),
    (None, 72, "estep_resp_split_band_kernel<8,4,3>", (2, 64), True),
    (None, 16, "estep_resp_kernel<2,8>", (2, 8), False),
    (None, 32, "estep_resp_kernel<2,16>", (2, 16), False),
    (None, 256, "estep_resp_kernel<4,64>", (4, 64), False),
    (None, 512, "estep_resp_kernel<8,64>", (8, 64), False),
    ("split", 16, "estep_resp_split_kernel<1,4,4>", (2, 8), True),
    ("split", 32, "estep_resp_split_kernel<2,4,4>", (2, 16), True),
    ("split", 48, "estep_resp_split_kernel<4,4,4>", (2, 32), True),
    ("split", 256, "estep_resp_kernel<4,64>", (4, 64), False),   # unsupported: falls through
    ("splitlds", 128, "estep_resp_split_kernel<8,12,3>", (2, 64), True),
    ("tile", 128, "estep_resp_tile_kernel<4,2,8,3>", (2, 64), False),
    ("mfma", 16, "estep_resp_mfma_kernel<1,4>", (2, 8), False),
    ("mfma", 128, "estep_resp_mfma_kernel<8,3>", (4, 32), False),
    ("mfma", 256, "estep_resp_mfma_kernel<16,2>", (4, 64), False),
    ("mfma", 512, "estep_resp_mfma_kernel<32,2>", (8, 64), False),
    ("legacy", 128, "estep_resp_kernel<4,32>", (4, 32), False),
]

# K -> (name("stats"), layout stats)
STATS = {
    16: ("estep_stats_kernel<2,8>", (2, 8)),
    32: ("estep_stats_kernel<2,16>", (2, 16)),
    48: ("estep_stats_kernel<2,32>", (2, 32)),
    72: ("estep_stats_tile_kernel<4,2>", (2, 64)),
    128: ("estep_stats_tile_kernel<4,2>", (2, 64)),
    256: ("estep_stats_tile_kernel<2,2,true>", (4, 64)),
    512: ("estep_stats_tile_kernel<4,2,true>", (8, 64)),
}

CASES = []
for _kernel, _K, _name, _layout, _split in ROWS:
    CASES.append((_kernel, None, _K, _name, _layout))
    if _split:   # SDMM_RESP_IMAGE=inline: "_inline" before "_kernel"
        CASES.append((_kernel, "inline", _K, _name.replace("_kernel<", "_inline_kernel<"), _layout))
    else:        # no effect on the other kernels
        CASES.append((_kernel, "inline", _K, _name, _layout))


@pytest.mark.parametrize("kernel,image,K,resp_name,resp_layout", CASES,
                         ids=[f"{c[0] or 'unset'}-{c[1] or 'unset'}-{c[2]}" for c in CASES])
def test_kernel_choice(pkg, gpu, monkeypatch, kernel, image, K, resp_name, resp_layout):
    for var, val in (("SDMM_RESP_KERNEL", kernel), ("SDMM_RESP_IMAGE", image)):
        if val is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, val)
    mix = pkg.SDMM(K)
    stats_name, stats_layout = STATS[K]
    lay = mix.layout()
    assert mix.kernel_name("resp") == resp_name
    assert mix.kernel_name("stats") == stats_name
    assert lay["resp"] == resp_layout
    assert lay["stats"] == stats_layout
