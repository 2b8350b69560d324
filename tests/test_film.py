"""CPU: the host film (sdmm_film_* with device = -1), the EXR reader and
combine_run against the numpy float32 restatement of tests/film_cases.py.

Per-pixel results (variance, resolve) are compared bit for bit.  The means
(pcv, mean pixel variance, the three errors) are fp64 sums in the library's
own fixed order; they are held to film_cases.sum_bound(n) against numpy's fp64
mean of the same float32 terms -- the distance between two orderings of a sum
of n non-negative terms, nothing tuned.
"""
import ctypes as C
import json
import shutil
import struct
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))
import film_cases as fc  # noqa: E402
from helpers import read_exr as helpers_read_exr  # noqa: E402

H, W = 29, 37            # 1073 pixels: four full chunks and a partial one
ITERS = range(7)
SPPS = (2, 3, 4, 7, 64)


def _passes(planted=True):
    return [fc.make_pass(H, W, 100 + i, planted) + (SPPS[i % len(SPPS)], i) for i in ITERS]


@pytest.mark.parametrize("spp", SPPS)
def test_variance_bitwise(pkg, spp):
    img, sqr = fc.make_pass(H, W, spp, planted=True)
    got = pkg.Film(W, H, device=-1).variance(img, sqr, spp)
    ref = fc.to_planes(fc.np_variance(fc.to_hwc(img), fc.to_hwc(sqr), spp))
    assert np.array_equal(fc.bits(got), fc.bits(ref))
    p = fc.planted_pixels(H * W)
    flat = got.reshape(3, -1)
    assert np.isnan(flat[0, p[0]]) and flat[2, p[2]] == 0.0 and flat[2, p[3]] == 2000.0


@pytest.mark.parametrize("shape", [(1, 1), (1, 255), (16, 16), (257, 1), (H, W), (300, 300)])
def test_pass_means_against_fp64_numpy(pkg, shape):
    h, w = shape
    img, sqr = fc.make_pass(h, w, 7, planted=False)
    film = pkg.Film(w, h, device=-1)
    st = film.add_pass(img, sqr, 4, 0)
    var = fc.np_variance(fc.to_hwc(img), fc.to_hwc(sqr), 4).astype(np.float64)
    print("pcv", st["pcv"], var.mean(axis=(0, 1)), "agg", st["mean_pixel_variance"], var.mean())
    assert fc.close(st["pcv"], var.mean(axis=(0, 1)), h * w)
    assert fc.close(st["mean_pixel_variance"], var.mean(), 3 * h * w)
    assert len(film) == 1 and film.pass_stats(0)["mean_pixel_variance"] == st["mean_pixel_variance"]


@pytest.mark.parametrize("planted", [False, True])
@pytest.mark.parametrize("mode", fc.MODES)
def test_combination_bitwise(pkg, mode, planted):
    film = pkg.Film(W, H, mode, first_iteration=4, device=-1)
    ref = fc.NumpyFilm(mode, 4)
    included = []
    for img, sqr, spp, it in _passes(planted):
        if not any(included):
            with pytest.raises(pkg.SDMMError, match="-3"):
                film.resolve()
        st = film.add_pass(img, sqr, spp, it)
        included.append(int(st["included"]))
        inc = ref.add_pass(fc.to_hwc(img), fc.to_hwc(sqr), spp, it, st["pcv"].astype(np.float32))
        assert inc == st["included"]
        if inc:
            assert np.array_equal(fc.bits(film.resolve()), fc.bits(fc.to_planes(ref.resolve()))), (mode, it)
    assert included == [0, 0, 0, 0, 1, 1, 1]
    final = film.resolve()
    if planted and mode != "uniform":
        assert np.isnan(final[0]).all()        # a NaN variance poisons its channel's weight
    else:
        assert np.isfinite(final[2]).all()
    film.reset()
    assert len(film) == 0
    with pytest.raises(pkg.SDMMError, match="-3"):
        film.resolve()


@pytest.mark.parametrize("mode", fc.MODES)
def test_constant_channel_nonfinite_pattern(pkg, mode):
    """sqr = img^2 * spp in channel 1: zero variance, weight 0, an infinite
    weight and inf / inf = NaN, as numpy gives."""
    film = pkg.Film(W, H, mode, first_iteration=0, device=-1)
    ref = fc.NumpyFilm(mode, 0)
    for i in range(2):
        img, sqr = fc.make_pass(H, W, 40 + i, planted=False)
        img[1] = 0.5
        sqr[1] = 0.0625        # (0.5 / 4)^2 * 4: sqr / spp == (img / spp)^2 exactly
        st = film.add_pass(img, sqr, 4, i)
        assert st["pcv"][1] == 0.0
        ref.add_pass(fc.to_hwc(img), fc.to_hwc(sqr), 4, i, st["pcv"].astype(np.float32))
    got, want = film.resolve(), fc.to_planes(ref.resolve())
    assert np.array_equal(fc.bits(got), fc.bits(want))
    if mode == "uniform":
        assert np.isfinite(got).all()
    else:       # var: w = pcv = 0; max_var: w = max(0, 0) = 0
        assert np.isnan(got[1]).all() and np.isfinite(got[0]).all() and np.isfinite(got[2]).all()


@pytest.mark.parametrize("mode", fc.MODES)
def test_errors_against_fp64_numpy(pkg, mode):
    gt = fc.make_truth(H, W, 5)
    film = pkg.Film(W, H, mode, first_iteration=1, device=-1)
    n = 3 * H * W
    for k, (img, sqr, spp, it) in enumerate(_passes(planted=False)[:3]):
        film.add_pass(img, sqr, spp, it)
        # INDIVIDUAL: the pass's own image
        e = film.errors(gt, img)
        t = fc.np_error_terms(fc.to_hwc(img), fc.to_hwc(gt))
        for name, term in zip(("MrSE", "MAPE", "SMAPE"), t):
            print(mode, it, "individual", name, e[name], term.astype(np.float64).mean())
            assert fc.close(e[name], term.astype(np.float64).mean(), n)
        if it < 1:
            with pytest.raises(pkg.SDMMError, match="-3"):
                film.errors(gt)
            continue
        # CUMULATIVE: the combined estimate
        e = film.errors(gt)
        t = fc.np_error_terms(fc.to_hwc(film.resolve()), fc.to_hwc(gt))
        for name, term in zip(("MrSE", "MAPE", "SMAPE"), t):
            print(mode, it, "cumulative", name, e[name], term.astype(np.float64).mean())
            assert fc.close(e[name], term.astype(np.float64).mean(), n)
            assert e[name] > 0


def test_errors_keep_a_nan(pkg):
    gt = fc.make_truth(H, W, 5)
    img, _ = fc.make_pass(H, W, 3, planted=True)
    e = pkg.Film(W, H, device=-1).errors(gt, img)
    assert all(np.isnan(e[k]) for k in ("MrSE", "MAPE", "SMAPE"))


def test_validation(pkg):
    lib = pkg.lib()
    h = C.c_void_p()

    def invalid(rc, word):
        assert rc == -1, rc
        assert word.encode() in lib.sdmm_last_error(), lib.sdmm_last_error()

    invalid(lib.sdmm_film_create(4, 4, 0, 4, -1, None), "NULL")
    invalid(lib.sdmm_film_create(0, 4, 0, 4, -1, C.byref(h)), "width or height")
    invalid(lib.sdmm_film_create(4, 0, 0, 4, -1, C.byref(h)), "width or height")
    invalid(lib.sdmm_film_create(-3, 4, 0, 4, -1, C.byref(h)), "width or height")
    invalid(lib.sdmm_film_create(1 << 14, (1 << 12) + 1, 0, 4, -1, C.byref(h)), "2^26")
    invalid(lib.sdmm_film_create(4, 4, 3, 4, -1, C.byref(h)), "mode")
    invalid(lib.sdmm_film_create(4, 4, -1, 4, -1, C.byref(h)), "mode")
    invalid(lib.sdmm_film_create(4, 4, 0, -1, -1, C.byref(h)), "first_iteration")
    assert not h.value
    assert lib.sdmm_film_create(4, 4, 0, 4, -1, C.byref(h)) == 0 and h.value
    a = np.ones((3, 4, 4), np.float32)
    st = pkg._FilmStats()
    er = pkg._FilmError()
    p = a.ctypes.data
    invalid(lib.sdmm_film_add_pass(None, p, p, 4, 0, None, C.byref(st)), "NULL")
    invalid(lib.sdmm_film_add_pass(h, None, p, 4, 0, None, C.byref(st)), "NULL")
    invalid(lib.sdmm_film_add_pass(h, p, None, 4, 0, None, C.byref(st)), "NULL")
    invalid(lib.sdmm_film_add_pass(h, p, p, 1, 0, None, C.byref(st)), "spp < 2")
    invalid(lib.sdmm_film_add_pass(h, p, p, 0, 0, None, C.byref(st)), "spp < 2")
    assert lib.sdmm_film_passes(h) == 0 and lib.sdmm_film_passes(None) == -1
    invalid(lib.sdmm_film_pass_stats(h, 0, C.byref(st)), "no such pass")
    invalid(lib.sdmm_film_pass_stats(None, 0, C.byref(st)), "NULL")
    invalid(lib.sdmm_film_pass_stats(h, 0, None), "NULL")
    invalid(lib.sdmm_film_resolve(None, p, None), "NULL")
    invalid(lib.sdmm_film_resolve(h, None, None), "NULL")
    assert lib.sdmm_film_resolve(h, p, None) == -3          # SDMM_E_STATE: nothing included yet
    invalid(lib.sdmm_film_errors(None, p, p, None, C.byref(er)), "NULL")
    invalid(lib.sdmm_film_errors(h, p, None, None, C.byref(er)), "NULL")
    invalid(lib.sdmm_film_errors(h, p, p, None, None), "NULL")
    assert lib.sdmm_film_errors(h, None, p, None, C.byref(er)) == -3
    invalid(lib.sdmm_film_variance(None, p, p, 4, p, None), "NULL")
    invalid(lib.sdmm_film_variance(h, None, p, 4, p, None), "NULL")
    invalid(lib.sdmm_film_variance(h, p, None, 4, p, None), "NULL")
    invalid(lib.sdmm_film_variance(h, p, p, 4, None, None), "NULL")
    invalid(lib.sdmm_film_variance(h, p, p, 1, p, None), "spp < 2")
    invalid(lib.sdmm_film_reset(None), "NULL")
    assert lib.sdmm_film_add_pass(h, p, p, 2, 9, None, None) == 0 and lib.sdmm_film_passes(h) == 1
    lib.sdmm_film_destroy(h)
    lib.sdmm_film_destroy(None)
    w, hh = C.c_int(), C.c_int()
    invalid(lib.sdmm_read_exr(None, C.byref(w), C.byref(hh), None, None, None, None), "invalid argument")
    invalid(lib.sdmm_read_exr(b"x.exr", None, C.byref(hh), None, None, None, None), "invalid argument")
    invalid(lib.sdmm_read_exr(b"/nonexistent/x.exr", C.byref(w), C.byref(hh), None, None, None, None), "cannot open")
    with pytest.raises(ValueError):
        pkg.Film(4, 4, "median", device=-1)


# ---- the EXR reader ----------------------------------------------------------
def _attr(name, typ, value):
    return name.encode() + b"\0" + typ.encode() + b"\0" + struct.pack("<i", len(value)) + value


def exr_bytes(planes, order=("B", "G", "R"), ptype=2, compression=0, window=None, extra=b"", drop_offsets=False):
    """An uncompressed scanline OpenEXR file of the named channels, in the
    listed order; returns (bytes, {section: its end position})."""
    data = {"R": planes[0], "G": planes[1], "B": planes[2], "A": planes[0] * 0 + 1}
    h, w = planes[0].shape
    chl = b"".join(c.encode() + b"\0" + struct.pack("<iiii", ptype, 0, 1, 1) for c in order) + b"\0"
    box = struct.pack("<4i", *(window or (0, 0, w - 1, h - 1)))
    head = struct.pack("<II", 20000630, 2)
    marks = {"version": len(head)}
    head += _attr("channels", "chlist", chl)
    marks["channels"] = len(head)
    head += _attr("compression", "compression", bytes([compression]))
    head += _attr("dataWindow", "box2i", box) + _attr("displayWindow", "box2i", box)
    head += _attr("lineOrder", "lineOrder", b"\0")
    head += _attr("spp", "int", struct.pack("<i", 7)) + _attr("iteration", "int", struct.pack("<i", 3))
    head += _attr("time", "float", struct.pack("<f", 2.5)) + extra
    marks["attributes"] = len(head)
    head += b"\0"
    marks["header"] = len(head)
    line = 8 + 4 * w * len(order)
    first = len(head) + 8 * h
    table = b"".join(struct.pack("<Q", first + line * y) for y in range(h))
    marks["table"] = first
    body = b""
    for y in range(h):
        body += struct.pack("<ii", y, 4 * w * len(order))
        marks.setdefault("line header", first + 8)
        for c in order:
            body += np.ascontiguousarray(data[c][y], np.float32).tobytes()
        marks.setdefault("first line", first + line)
    return head + table + body, marks


def malformed_family(planes):
    """(name, bytes) of files sdmm_read_exr must refuse (tests/cpp/exr_check.cpp
    runs over the same files)."""
    good, marks = exr_bytes(planes)
    h, w = planes[0].shape
    fam = [("truncated after " + k, good[:v]) for k, v in marks.items()]
    fam += [("truncated inside " + k, good[:v - 3]) for k, v in marks.items()]
    fam.append(("truncated before the last float", good[:-1]))
    fam.append(("empty", b""))
    fam.append(("not exr", b"\0" * 64))
    t = marks["header"]
    fam.append(("offset past the end", good[:t] + struct.pack("<Q", len(good) + 100) + good[t + 8:]))
    fam.append(("offset at the last byte", good[:t] + struct.pack("<Q", len(good) - 1) + good[t + 8:]))
    fam.append(("offset huge", good[:t] + struct.pack("<Q", 2 ** 64 - 4) + good[t + 8:]))
    fam.append(("offset into the header", good[:t] + struct.pack("<Q", 8) + good[t + 8:]))
    fam.append(("negative data window", exr_bytes(planes, window=(0, 0, -5, h - 1))[0]))
    fam.append(("inverted data window", exr_bytes(planes, window=(w, 0, 0, h - 1))[0]))
    fam.append(("huge data window", exr_bytes(planes, window=(0, 0, 2 ** 31 - 1, 2 ** 31 - 1))[0]))
    fam.append(("window wider than the data", exr_bytes(planes, window=(0, 0, 4 * w, h - 1))[0]))
    fam.append(("window taller than the data", exr_bytes(planes, window=(0, 0, w - 1, 40 * h))[0]))
    fam.append(("compression set", exr_bytes(planes, compression=3)[0]))
    fam.append(("HALF channel", exr_bytes(planes, ptype=1)[0]))
    fam.append(("missing channel", exr_bytes(planes, order=("B", "R"))[0]))
    fam.append(("tiled", good[:4] + struct.pack("<I", 2 | 0x200) + good[8:]))
    fam.append(("attribute longer than the file",
                exr_bytes(planes, extra=b"x\0string\0" + struct.pack("<i", 2 ** 31 - 1))[0]))
    fam.append(("negative attribute size", exr_bytes(planes, extra=b"x\0string\0" + struct.pack("<i", -8))[0]))
    bad_y = bytearray(good)
    struct.pack_into("<i", bad_y, marks["table"], h + 5)
    fam.append(("scanline outside the window", bytes(bad_y)))
    bad_n = bytearray(good)
    struct.pack_into("<i", bad_n, marks["table"] + 4, 4 * w)
    fam.append(("scanline of the wrong size", bytes(bad_n)))
    return fam


@pytest.fixture(scope="module")
def planes():
    return fc.make_pass(5, 7, 1, planted=True)[0]


def test_read_exr_round_trip(pkg, planes, tmp_path):
    path = tmp_path / "a.exr"
    pkg.write_exr(path, planes, spp=6, iteration=12, time=1.25)
    got, attrs = pkg.read_exr(path)
    assert np.array_equal(got.view(np.uint32), planes.view(np.uint32))     # NaN payload included
    assert attrs == {"spp": 6, "iteration": 12, "time": 1.25}
    ref, ra = helpers_read_exr(path)
    assert np.array_equal(fc.bits(got), fc.bits(ref))
    assert (ra["spp"], ra["iteration"], ra["time"]) == (6, 12, 1.25)


@pytest.mark.parametrize("order", [("R", "G", "B"), ("G", "R", "B"), ("A", "B", "G", "R"), ("B", "A", "R", "G")])
def test_read_exr_channel_order(pkg, planes, tmp_path, order):
    path = tmp_path / "o.exr"
    path.write_bytes(exr_bytes(planes, order=order)[0])
    got, attrs = pkg.read_exr(path)
    assert np.array_equal(got.view(np.uint32), planes.view(np.uint32))
    assert attrs == {"spp": 7, "iteration": 3, "time": 2.5}


def test_read_exr_refuses_malformed_files(pkg, planes, tmp_path):
    lib = pkg.lib()
    fam = malformed_family(planes)
    assert len(fam) >= 30
    for k, (name, data) in enumerate(fam):
        path = tmp_path / f"bad{k}.exr"
        path.write_bytes(data)
        w, h = C.c_int(), C.c_int()
        rc = lib.sdmm_read_exr(str(path).encode(), C.byref(w), C.byref(h), None, None, None, None)
        if rc == 0:   # the header may be whole: planes of the size it states, and the data is refused
            n = 3 * w.value * h.value
            assert 0 < n < 1 << 20, name
            out = np.zeros(n + 16, np.float32)
            rc = lib.sdmm_read_exr(str(path).encode(), C.byref(w), C.byref(h), out.ctypes.data, None, None, None)
            assert not out[n:].any(), name
        assert rc == -1, name
        assert lib.sdmm_last_error(), name


def test_exr_check_program(pkg, planes, tmp_path):
    """tests/cpp/exr_check.cpp, a program of its own over the library: the good
    file reads back, every malformed one is refused."""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler on this machine")
    good = tmp_path / "good.exr"
    pkg.write_exr(good, planes, spp=6, iteration=12, time=1.25)
    names = []
    for k, (_, data) in enumerate(malformed_family(planes)):
        names.append(tmp_path / f"bad{k}.exr")
        names[-1].write_bytes(data)
    lib = ROOT / "sdmm-mitsuba_amd" / "lib"
    exe = tmp_path / "exr_check"
    subprocess.run([cxx, "-std=c++17", "-O1", f"-I{ROOT / 'include'}", str(ROOT / "tests" / "cpp" / "exr_check.cpp"),
                    f"-L{lib}", "-lsdmm_amd", f"-Wl,-rpath,{lib}", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), str(good), *map(str, names)], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0
    assert f"exr_check ok: 1 read, {len(names)} refused" in r.stdout


# ---- combine_run and RunStats ------------------------------------------------
@pytest.mark.parametrize("mode", fc.MODES)
def test_combine_run(pkg, tmp_path, mode):
    gt = fc.make_truth(H, W, 5)
    film = pkg.Film(W, H, mode, device=-1)
    rows, want = [], {"mean_pixel_variance": [], "MrSE": [], "MAPE": [], "SMAPE": []}
    for img, sqr, spp, it in _passes(planted=False):
        pkg.write_exr(tmp_path / f"iteration{it:05d}.exr", img, spp=spp, iteration=it, time=0.5 * it)
        pkg.write_exr(tmp_path / f"iteration_sqr{it:05d}.exr", sqr, spp=spp, iteration=it, time=0.5 * it)
        rows.append({"iteration": it, "elapsed_seconds": 0.25 + it, "total_elapsed_seconds": 3.0 * it,
                     "mean_path_length": 2.5, "spp": spp, "total_spp": 9})
        st = film.add_pass(img, sqr, spp, it)
        want["mean_pixel_variance"].append(st["mean_pixel_variance"])
        e = film.errors(gt, None if it >= 4 else img)
        for k in ("MrSE", "MAPE", "SMAPE"):
            want[k].append(e[k])
    (tmp_path / "stats.json").write_text(json.dumps(rows))
    (tmp_path / "notes.txt").write_text("not a pass")
    res = pkg.combine_run(tmp_path, mode, ground_truth=gt)
    for k, v in want.items():
        assert res[k] == v, k
    assert res["included"] == [False] * 4 + [True] * 3
    assert res["out"] == str(tmp_path / "combined.exr")
    assert np.array_equal(fc.bits(pkg.read_exr(res["out"])[0]), fc.bits(film.resolve()))
    out = json.loads((tmp_path / "stats.json").read_text())
    for row, src, v in zip(out, rows, want["mean_pixel_variance"]):
        assert row["mean_pixel_variance"] == v and row["ttuv"] == v * src["elapsed_seconds"]
        assert {k: row[k] for k in src} == src
    # a ground truth by path, another output path
    pkg.write_exr(tmp_path / "gt.exr", gt)
    res2 = pkg.combine_run(tmp_path, mode, ground_truth=tmp_path / "gt.exr", out=tmp_path / "elsewhere.exr")
    assert res2["SMAPE"] == want["SMAPE"] and (tmp_path / "elsewhere.exr").exists()


RUNSTATS_SRC = r"""
#include "sdmm_amd.hpp"
int main(int argc, char** argv) {
    sdmm_amd::RunStats a, b;
    for (int i = 0; i < 3; ++i) {
        a.push(i, 0.5 + i, 1.5 * i, 2.25, 4, 4 * (i + 1));
        b.push(i, 0.5 + i, 1.5 * i, 2.25, 4, 4 * (i + 1));
    }
    a.write(argv[1]);
    b.set_mean_pixel_variance(1, 0.125);
    b.write(argv[2]);
    // the film's C++ mirror on the host
    sdmm_amd::Film film(2, 2, SDMM_FILM_VAR, 0, -1);
    const float img[12] = {1, 2, 3, 4, 1, 2, 3, 4, 1, 2, 3, 4}, sqr[12] = {2, 8, 18, 32, 2, 8, 18, 32, 2, 8, 18, 32};
    const sdmm_film_stats st = film.add_pass(img, sqr, 4, 0);
    float out[12];
    film.resolve(out);
    const sdmm_film_error e = film.errors(out, out);
    return (st.included == 1 && film.passes() == 1 && out[0] == 1.0f && e.smape == 0.0) ? 0 : 1;
}
"""


def _runstats_text(rows):
    """RunStats::write's layout: nlohmann's dump(4) with sorted keys, doubles as %.17g."""
    out = []
    for r in rows:
        keys = sorted(r)
        out.append("    {\n" + ",\n".join(
            f'        "{k}": ' + (str(r[k]) if isinstance(r[k], int) else "%.17g" % r[k]) for k in keys) + "\n    }")
    return "[\n" + ",\n".join(out) + "\n]\n"


def test_runstats_text_unchanged_without_variance(tmp_path):
    """RunStats::write without a variance set writes today's text byte for
    byte; a row with one carries the key where nlohmann's sorted dump puts it."""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler on this machine")
    src = tmp_path / "rs.cpp"
    src.write_text(RUNSTATS_SRC)
    lib = ROOT / "sdmm-mitsuba_amd" / "lib"
    exe = tmp_path / "rs"
    subprocess.run([cxx, "-std=c++17", f"-I{ROOT / 'sdmm-mitsuba_amd' / 'host'}", f"-I{ROOT / 'include'}", str(src),
                    f"-L{lib}", "-lsdmm_amd", f"-Wl,-rpath,{lib}", "-o", str(exe)], check=True)
    subprocess.run([str(exe), str(tmp_path / "a.json"), str(tmp_path / "b.json")], check=True, timeout=60)
    rows = [{"elapsed_seconds": 0.5 + i, "iteration": i, "mean_path_length": 2.25, "spp": 4,
             "total_elapsed_seconds": 1.5 * i, "total_spp": 4 * (i + 1)} for i in range(3)]
    a = (tmp_path / "a.json").read_text()
    assert a == _runstats_text(rows)
    assert "mean_pixel_variance" not in a and json.loads(a) == rows
    rows[1]["mean_pixel_variance"] = 0.125
    b = (tmp_path / "b.json").read_text()
    assert b == _runstats_text(rows) and json.loads(b) == rows
