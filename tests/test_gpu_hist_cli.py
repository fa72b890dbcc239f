"""GPU: vr_cli --histogram writes the library's value histogram (include/vr/vr_hist.h) as JSON in
place of the image, and --window renders with the percentile window of that histogram."""
import json
import os
import subprocess

import numpy as np
import pytest

import synth
import vr_amd

pytestmark = pytest.mark.gpu
CLI = os.path.join(os.path.dirname(vr_amd.LIB_PATH), "vr_cli")


def g9(x):
    """%.9g and back: what the JSON holds of an f32 (9 digits identify it)."""
    return float("%.9g" % float(x))


@pytest.mark.parametrize("spec,nbins,lo,hi", [("64", 64, None, None), ("100:0.1:0.9", 100, 0.1, 0.9)])
def test_cli_histogram(gpu, tmp_path, spec, nbins, lo, hi):
    out = str(tmp_path / "h.json")
    rp = vr_amd.OffscreenPass(32, 24)
    try:
        window = rp.generate_volume((40, 40, 40), np.float32, seed=2024)
        bins, info = rp.histogram(nbins, lo, hi)
        lo, hi = (window[0] if lo is None else lo), (window[1] if hi is None else hi)
    finally:
        rp.close()
    r = subprocess.run([CLI, "synthetic:40", out, "--histogram", spec], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    got = json.load(open(out))
    assert list(got) == ["nbins", "lo", "hi", "bins", "voxels", "below", "above", "nan", "vmin", "vmax"]
    assert got["nbins"] == nbins and got["bins"] == [int(b) for b in bins]
    assert (got["lo"], got["hi"]) == (g9(np.float32(lo)), g9(np.float32(hi)))
    assert np.float32(got["lo"]) == np.float32(lo) and np.float32(got["hi"]) == np.float32(hi)
    for k in ("voxels", "below", "above", "nan"):
        assert got[k] == int(info[k]), k
    assert got["voxels"] == 64000 == sum(got["bins"]) + got["below"] + got["above"] + got["nan"]
    assert (np.float32(got["vmin"]), np.float32(got["vmax"])) == (info["vmin"], info["vmax"])
    assert (got["below"] > 0) == (spec != "64") and np.count_nonzero(bins) > 8


def test_cli_window(gpu, tmp_path):
    w, h = 96, 64
    out = str(tmp_path / "f.ppm")
    cam = vr_amd.make_camera(radius=2.0, rotate=(100.0, 60.0)).to_vr_camera()
    rp = vr_amd.OffscreenPass(w, h)
    try:
        lo, hi = rp.generate_volume((40, 40, 40), np.float32, seed=2024)
        rp.transfer_function_changed(synth.tf2())
        plain = rp.render(cam, vr_amd.default_params(), vr_amd.OUT_RGBA8)
        _, info = rp.histogram(1, lo, hi)
        bins, _ = rp.histogram(vr_amd.HIST_MAX_BINS, info["vmin"], info["vmax"])
        rp.value_range_changed(*vr_amd.hist_window(bins, info["vmin"], info["vmax"], 0.05, 0.95))
        ref = rp.render(cam, vr_amd.default_params(), vr_amd.OUT_RGBA8)
    finally:
        rp.close()
    r = subprocess.run([CLI, "synthetic:40", out, "--size", f"{w}x{h}", "--radius", "2", "--rotate",
                        "100,60", "--tf", "demo", "--window", "0.05:0.95"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    data = open(out, "rb").read().split(b"\n", 3)
    assert data[1] == f"{w} {h}".encode()
    img = np.frombuffer(data[3], np.uint8).reshape(h, w, 3)
    assert np.array_equal(img, ref[..., :3]) and not np.array_equal(img, plain[..., :3])


def test_cli_refuses_bad_arguments(gpu, tmp_path):
    for opt, specs in (("--histogram", ("0", "4097", "8:1:1", "8:0", "x", "8:0:inf", "7.5")),
                       ("--window", ("0.5", "0.5:0.5", "-0.1:1", "0:1.5", "a:b", "0:1:2"))):
        for spec in specs:
            r = subprocess.run([CLI, "synthetic:8", str(tmp_path / "x.out"), opt, spec],
                               capture_output=True, text=True, timeout=120)
            assert r.returncode == 2 and opt in r.stderr, (opt, spec, r.stderr)
            assert not os.path.exists(tmp_path / "x.out")
