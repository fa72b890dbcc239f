"""CPU: the render-mode ABI (include/vr/vr_modes.h) and the reference helper's MIP mode.

No compute calls (no GPU in the build container): exported symbols, argument checks, the
unchanged ABI version, the helper's own loop pinned against the C oracle, and the C++ shim's
render_mode_changed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import proj_ref
import pyoracle
import synth
import vr_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "volumetric-renderer_amd", "lib")

SLICE = ((0.2, 0.0, 0.1), (0.8, 1.0, 0.9))
W, H = 32, 24


def scene(camname, smin=(0, 0, 0), smax=(1, 1, 1), tf=None, vol=None, w=W, h=H, **params):
    vol = synth.gaussians_numpy((20, 18, 22), seed=11) if vol is None else vol
    ds = synth.dataset(vol)
    cam = synth.camera(camname).to_vr_camera()
    p = vr_amd.default_params(**params)
    return pyoracle.Scene.from_params(vol, ds.vmin, ds.vmax, synth.tf_color() if tf is None else tf,
                                      cam, w, h, p, smin=smin, smax=smax)


def declared(header):
    src = open(os.path.join(ROOT, "include", "vr", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(vr_[a-z0-9_]+)\s*\(", src))


def test_modes_header_symbols_are_exported_and_bound():
    names = declared("vr_modes.h")
    assert names == {"vr_set_render_mode", "vr_get_render_mode"}
    out = subprocess.run(["nm", "-D", "--defined-only", vr_amd.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert not names - exported, names - exported
    assert names == set(vr_amd.MODES_SYMBOLS)
    assert (vr_amd.MODE_COMPOSITE, vr_amd.MODE_MIP) == (0, 1)
    src = open(os.path.join(ROOT, "include", "vr", "vr_modes.h")).read()
    assert re.search(r"VR_MODE_COMPOSITE\s*=\s*0\s*,\s*VR_MODE_MIP\s*=\s*1", src)


def test_mode_entry_points_reject_null():
    L = vr_amd.lib()
    assert L.vr_set_render_mode(None, 1) == -22
    assert L.vr_get_render_mode(None, None) == -22
    m = C.c_int(7)
    assert L.vr_get_render_mode(None, C.byref(m)) == -22 and m.value == 7


def test_abi_version_is_unchanged():
    assert vr_amd.lib().vr_abi_version() == 9 == vr_amd.ABI_VERSION
    assert "VR_ABI_VERSION 9" in open(os.path.join(ROOT, "include", "vr", "vr.h")).read()
    assert vr_amd.KNOBS["mip_inflight"] == 10


@pytest.mark.parametrize("camname,box,rays,empty", [("rotA", ((0, 0, 0), (1, 1, 1)), 443, None),
                                                    ("fill_oblique", SLICE, 698, 303)])
def test_reference_loop_reproduces_the_oracle_composite(camname, box, rays, empty):
    """proj_ref's loop in composite mode is the C oracle bit for bit: same frame, same counters."""
    sc = scene(camname, smin=box[0], smax=box[1])
    ref, st = sc.render()
    got, gs = proj_ref.render(sc, mode="composite")
    assert st["rays"] == rays == gs["rays"]
    assert gs["steps"] == st["steps"] and gs["samples"] == st["samples"]
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    if empty is not None:  # rays that cross the cube but never the slice box keep the clear colour
        clear = np.array([0.11, 0.11, 0.11, 1.0], np.float32)
        mip, ms = proj_ref.render(sc, mode="mip")
        assert ms == gs
        untouched = np.all(mip == clear, axis=-1).sum() - (W * H - rays)
        assert untouched == empty


def test_reference_mip_closed_form():
    """A constant volume of value 1 under a one-texel TF (c, a): every ray with an in-slab sample
    is c a a + clear (1 - a), alpha a^2 + (1 - a) -- checked in float64 to f32 rounding."""
    vol = np.ones((6, 5, 7), np.float32)
    tf = np.array([0x80FFFFFF], np.uint32)  # white, alpha 128/255
    cam = synth.camera("rotA").to_vr_camera()
    sc = pyoracle.Scene.from_params(vol, 0.0, 1.0, tf, cam, 16, 12, vr_amd.default_params())
    img, st = proj_ref.render(sc, mode="mip")
    a = 128.0 / 255.0
    hit = img[..., 3] != 1.0
    assert 0 < hit.sum() <= st["rays"]
    assert np.allclose(img[hit][:, 3], a * a + 1 - a, rtol=0, atol=1e-6)
    assert np.allclose(img[hit][:, :3], a * a + 0.11 * (1 - a), rtol=0, atol=1e-6)
    assert np.all(img[~hit] == np.array([0.11, 0.11, 0.11, 1.0], np.float32))


def test_shim_compiles_with_render_mode_changed(tmp_path):
    src = str(tmp_path / "vr_shim_mode.cpp")
    exe = str(tmp_path / "vr_shim_mode")
    with open(src, "w") as f:
        f.write(r"""
#include <vr/offscreen_pass_hip.hpp>
#include <cstdio>
int main(int argc, char **)
{
    static_assert(VR_MODE_COMPOSITE == 0 && VR_MODE_MIP == 1, "vr_modes.h");
    if (argc > 1) {  // never taken in the CPU test: needs a device
        Vol::Rendering::Hip::OffscreenPass pass(8, 8);
        pass.render_mode_changed(VR_MODE_MIP);
        return pass.render_mode() == VR_MODE_MIP ? 0 : 1;
    }
    std::printf("%d\n", vr_set_render_mode(nullptr, VR_MODE_MIP));
    return 0;
}
""")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src,
                        "-o", exe, "-L", LIBDIR, "-lvr_amd", "-Wl,-rpath," + LIBDIR],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip() == "-22"
