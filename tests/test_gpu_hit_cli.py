"""GPU: vr_cli --pick X,Y --hit KIND[:THRESHOLD] prints the hit record of one framebuffer pixel
(include/vr/vr_hit.h) as one JSON line in place of the image: the reference's record
(tests/hit_ref.py, on the generated volume read back) for a hit, step -1 for a miss."""
import json
import os
import subprocess

import numpy as np
import pytest

import hit_ref
import pyoracle
import synth
import vr_amd

pytestmark = pytest.mark.gpu
CLI = os.path.join(os.path.dirname(vr_amd.LIB_PATH), "vr_cli")
W, H, N = 32, 24, 20
ISO_F, THRESHOLD = 0.3, 0.9
_walk = {}


def g9(x):
    """%.9g and back: what the JSON holds of an f32 (9 digits identify it)."""
    return float("%.9g" % float(x))


def walk():
    """The reference records of the CLI's scene, once per session."""
    if not _walk:
        rp = vr_amd.OffscreenPass(W, H)
        try:
            lo, hi = rp.generate_volume((N, N, N), np.float32, seed=2024)
            vol = rp.read_volume()
        finally:
            rp.close()
        iso = np.float32(lo + ISO_F * (hi - lo))
        cam = vr_amd.make_camera(radius=2.0, rotate=(100.0, 60.0)).to_vr_camera()
        scene = pyoracle.Scene.from_params(vol, lo, hi, synth.tf2(), cam, W, H, vr_amd.default_params())
        _walk["w"] = (hit_ref.walk(scene, iso, (THRESHOLD,)), iso)
    return _walk["w"]


def run(tmp_path, px, py, hit, iso):
    out = tmp_path / "never.ppm"
    r = subprocess.run([CLI, f"synthetic:{N}", str(out), "--size", f"{W}x{H}", "--radius", "2", "--rotate",
                        "100,60", "--tf", "demo", "--iso", repr(float(iso)), "--pick", f"{px},{py}", "--hit", hit],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert not out.exists()
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    got = json.loads(lines[0])
    assert list(got) == ["pos", "depth", "value", "step"]
    return got


@pytest.mark.parametrize("hit,key", [("max", "max"), ("iso", "iso"),
                                     (f"opacity:{THRESHOLD}", ("opacity", float(np.float32(THRESHOLD))))])
def test_cli_pick(gpu, tmp_path, hit, key):
    w, iso = walk()
    rec, hits = w.records[key], w.hits(key)
    assert hits.sum() >= 30 and (~hits).sum() >= 30
    at = np.argwhere(hits)
    py, px = at[len(at) // 2]
    got = run(tmp_path, px, py, hit, iso)
    r = rec[py, px]
    assert got["step"] == int(r["step"]) >= 0
    assert got["pos"] == [g9(x) for x in r["pos"]] and got["depth"] == g9(r["depth"])
    assert got["value"] == g9(r["value"])
    assert [np.float32(x) for x in got["pos"]] == list(r["pos"]) and np.float32(got["depth"]) == r["depth"]
    py, px = np.argwhere(~hits)[0]
    got = run(tmp_path, px, py, hit, iso)
    assert got == {"pos": [0.0, 0.0, 0.0], "depth": float("inf"), "value": 0.0, "step": -1}


def test_cli_refuses_bad_arguments(gpu, tmp_path):
    for args in (["--pick", "3,4"], ["--hit", "max"], ["--pick", "3", "--hit", "max"],
                 ["--pick", "3,4,5", "--hit", "max"], ["--pick", "3,4", "--hit", "average"],
                 ["--pick", "3,4", "--hit", "opacity:0"], ["--pick", "3,4", "--hit", "opacity:1.5"],
                 ["--pick", "3,4", "--hit", "opacity:x"], ["--pick", "3,4", "--hit", "max:0.5:1"]):
        r = subprocess.run([CLI, "synthetic:8", str(tmp_path / "x.out"), *args], capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 2 and "--pick" in r.stderr, (args, r.stderr)
    # a pixel beyond the framebuffer is the library's refusal
    r = subprocess.run([CLI, "synthetic:8", str(tmp_path / "x.out"), "--size", "32x24", "--pick", "32,0",
                        "--hit", "entry"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "beyond the framebuffer" in r.stderr
    assert not os.path.exists(tmp_path / "x.out")
