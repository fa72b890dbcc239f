"""GPU: vr_cli --mpr writes the library's multi-planar reformat image (include/vr/vr_mpr.h)
instead of the 3D frame."""
import os
import subprocess

import numpy as np
import pytest

import synth
import vr_amd

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("spec,axis,ns,spacing,op", [
    ("axial:0.37", vr_amd.AXIS_AXIAL, 1, 0.0, vr_amd.OP_MAX),
    ("coronal:0.6:5:0.01:mean", vr_amd.AXIS_CORONAL, 5, 0.01, vr_amd.OP_MEAN),
])
def test_cli_mpr(gpu, tmp_path, spec, axis, ns, spacing, op):
    cli = os.path.join(os.path.dirname(vr_amd.LIB_PATH), "vr_cli")
    w, h = 96, 64
    out = str(tmp_path / "f.ppm")
    rp = vr_amd.OffscreenPass(32, 24)  # the image's size is the plane's, not the framebuffer's
    try:
        rp.generate_volume((40, 40, 40), np.float32, seed=2024)
        rp.transfer_function_changed(synth.tf2())
        pos = float(spec.split(":")[1])
        ref = rp.render_mpr(vr_amd.axis_plane(axis, pos, w, h, ns, spacing, op), None, vr_amd.OUT_RGBA8)
        rp.framebuffer_size_changed(w, h)
        frame = rp.render(vr_amd.make_camera(radius=2.0, rotate=(100.0, 60.0)).to_vr_camera(),
                          vr_amd.default_params(), vr_amd.OUT_RGBA8)
    finally:
        rp.close()
    r = subprocess.run([cli, "synthetic:40", out, "--size", f"{w}x{h}", "--radius", "2", "--rotate",
                        "100,60", "--tf", "demo", "--mpr", spec], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    data = open(out, "rb").read().split(b"\n", 3)
    assert data[1] == f"{w} {h}".encode()
    img = np.frombuffer(data[3], np.uint8).reshape(h, w, 3)
    assert np.array_equal(img, ref[..., :3]) and not np.array_equal(img, frame[..., :3])
    assert len(np.unique(img.reshape(-1, 3), axis=0)) > 8


def test_cli_refuses_a_bad_mpr_argument(gpu, tmp_path):
    cli = os.path.join(os.path.dirname(vr_amd.LIB_PATH), "vr_cli")
    for spec in ("oblique:0.5", "axial", "axial:0.5:3", "axial:0.5:0:0.01:max", "axial:0.5:3:0.01:median"):
        r = subprocess.run([cli, "synthetic:8", str(tmp_path / "x.ppm"), "--mpr", spec],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "--mpr" in r.stderr, (spec, r.stderr)
        assert not os.path.exists(tmp_path / "x.ppm")
