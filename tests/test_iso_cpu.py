"""CPU: the isosurface ABI (include/vr/vr_iso.h), the ISO kernel family's names and the
reference helper tests/iso_ref.py.

No compute calls (no GPU in the build container): exported symbols, argument checks, the
unchanged ABI version and composite code hash, the helper's loop, gradient and Phong pinned
against the C oracle, the names resolve_variant yields for mode 3 against the kernels the
library carries, and the C++ shim's isovalue_changed."""
import ctypes as C
import itertools
import json
import os
import re
import subprocess

import numpy as np
import pytest

import iso_ref
import pyoracle
import synth
import vr_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "volumetric-renderer_amd", "lib")

SLICE = ((0.2, 0.0, 0.1), (0.8, 1.0, 0.9))
FULL = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
W, H = 32, 24


def declared(header):
    src = open(os.path.join(ROOT, "include", "vr", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(vr_[a-z0-9_]+)\s*\(", src))


# ---- 1. the header, the exports, the binding -------------------------------------------------
def test_iso_header_symbols_are_exported_and_bound():
    names = declared("vr_iso.h")
    assert names == {"vr_set_isovalue", "vr_get_isovalue"}
    out = subprocess.run(["nm", "-D", "--defined-only", vr_amd.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert not names - exported, names - exported
    assert names == set(vr_amd.ISO_SYMBOLS)
    assert vr_amd.MODE_ISO == 3
    src = open(os.path.join(ROOT, "include", "vr", "vr_modes.h")).read()
    assert re.search(r"VR_MODE_MIP\s*=\s*1\s*,\s*VR_MODE_ISO\s*=\s*3", src)
    assert "vr_modes.h" in open(os.path.join(ROOT, "include", "vr", "vr_iso.h")).read()
    assert vr_amd.lib().vr_abi_version() == 9 == vr_amd.ABI_VERSION
    assert "VR_ABI_VERSION 9" in open(os.path.join(ROOT, "include", "vr", "vr.h")).read()


# ---- 2. argument checks without a device -------------------------------------------------------
def test_iso_entry_points_reject_null():
    L = vr_amd.lib()
    assert L.vr_set_isovalue(None, C.c_float(0.5)) == -22
    assert L.vr_get_isovalue(None, None) == -22
    v = C.c_float(7.0)
    assert L.vr_get_isovalue(None, C.byref(v)) == -22 and v.value == 7.0
    assert L.vr_set_render_mode(None, 3) == -22


# ---- 3. the helper is pinned by the C oracle ---------------------------------------------------
@pytest.mark.parametrize("camname,box,rays", [("rotA", FULL, 443), ("fill_oblique", SLICE, 698)])
def test_reference_loop_reproduces_the_shaded_oracle_composite(camname, box, rays):
    """iso_ref's loop in composite mode with its own gradient and Phong restatement is the C
    oracle bit for bit (shading = 1, exact_gradient = 1): same frame, same counters."""
    vol = synth.gaussians_numpy((20, 18, 22), seed=11)
    ds = synth.dataset(vol)
    p = vr_amd.default_params(shading=1, exact_gradient=1)
    sc = pyoracle.Scene.from_params(vol, ds.vmin, ds.vmax, synth.tf_color(),
                                    synth.camera(camname).to_vr_camera(), W, H, p,
                                    smin=box[0], smax=box[1])
    ref, st = sc.render()
    got, gs, hit_step, cap = iso_ref.render(sc, mode="composite")
    assert st["rays"] == rays == gs["rays"]
    assert gs["steps"] == st["steps"] and gs["samples"] == st["samples"]
    assert gs["shaded_samples"] == st["shaded_samples"] > 0
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert np.all(hit_step == -1) and not cap.any()


def test_reference_iso_small_properties():
    """The helper's own ISO loop on a half-space volume: the hit step is monotone in the
    isovalue, caps appear exactly when the slice box cuts the solid half open."""
    n = 12
    vol = np.zeros((n, n, n), np.float32)
    vol[:, :, n // 2:] = 1.0
    cam = synth.camera("rotA").to_vr_camera()
    p = vr_amd.default_params(shading=1)
    sc = pyoracle.Scene.from_params(vol, 0.0, 1.0, synth.tf_color(), cam, 16, 12, p)
    img, st, hs, cap = iso_ref.render(sc, iso=0.5)
    img2, st2, hs2, _ = iso_ref.render(sc, iso=0.9)
    hit = hs >= 0
    assert 0 < hit.sum() < st["rays"] and st["shaded_samples"] == hit.sum()
    assert np.all(hs2[hs2 >= 0] >= hs[hs2 >= 0]) and not np.any((hs2 >= 0) & ~hit)
    assert np.all(img[hit][:, 3] == 1.0)
    assert np.all(img[~hit] == np.array([0.11, 0.11, 0.11, 1.0], np.float32))
    cut = pyoracle.Scene.from_params(vol, 0.0, 1.0, synth.tf_color(), cam, 16, 12, p,
                                     smin=(0.7, 0.0, 0.0), smax=(1.0, 1.0, 1.0))
    _, _, hs3, cap3 = iso_ref.render(cut, iso=0.5)
    assert (hs3 >= 0).sum() > 0 and np.array_equal(cap3, hs3 >= 0)  # every hit is at the cut


# ---- 4. variant names for mode 3 ---------------------------------------------------------------
ST_F32, QUAD, ALT, PLAIN, STENCIL = 4, 0x10, 0x20, 0x100, 0x200
BASE_TYPES = {0: "unsigned char", 1: "signed char", 2: "unsigned short", 3: "short", 4: "float",
              0 | QUAD: "vr::Quad8<unsigned char>", 1 | QUAD: "vr::Quad8<signed char>"}
LAYOUTS = list(BASE_TYPES) + [ST_F32 | ALT, ST_F32 | PLAIN, ST_F32 | STENCIL]
NS = "void vr::(anonymous namespace)::"


def expected_iso_name(layout, count, skip, k):
    if layout not in BASE_TYPES:
        return None
    if count:
        k = 1
    elif k not in (1, 2, 4):
        return None
    flags = "".join(", true" if f else ", false" for f in (count, skip))
    return f"{NS}iso_kernel<{BASE_TYPES[layout]}{flags}, {k}>(vr::MarchParams, vr::IsoArgs)"


def test_iso_variant_names_are_the_built_kernels():
    reachable = set()
    for layout, count, skip, k, shade in itertools.product(LAYOUTS, (0, 1), (0, 1), (0, 1, 2, 3, 4, 8),
                                                           (0, 1)):
        got = vr_amd.variant_name(layout=layout, mode=vr_amd.MODE_ISO, shade=shade, count=count,
                                  skip=skip, field=0, field_half=0, pipeline=0, tf_n=256, pair=0,
                                  mip_inflight=k)
        assert got == expected_iso_name(layout, count, skip, k), (layout, count, skip, k)
        if got is not None:
            reachable.add(got)
    assert len(reachable) == 7 * 2 * 4  # 7 layouts x skip x (K = 1, 2, 4 and the counting kernel)
    kd = sorted(name[:-3].decode() for name, _ in vr_amd.code_object_symbols()
                if name.endswith(b".kd"))
    dem = subprocess.run(["c++filt"], input="\n".join(kd), capture_output=True, text=True,
                         check=True).stdout.split("\n")
    built = {d for d in dem if "::iso_kernel<" in d}
    assert reachable - built == set()
    assert built - reachable == set()
    # mode 2 stays unassigned: no kernel serves it as a range mode
    assert "iso_kernel" not in (vr_amd.variant_name(layout=4, mode=2, shade=0, count=0, skip=0, field=0,
                                                    field_half=0, pipeline=0, tf_n=256, pair=0,
                                                    mip_inflight=2) or "")


def test_composite_code_hash_is_unchanged():
    want = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))["c3"]["code_hash"]
    assert vr_amd.kernel_code_hash() == want


# ---- 5. the shim ------------------------------------------------------------------------------
def test_shim_compiles_with_isovalue_changed(tmp_path):
    src = str(tmp_path / "vr_shim_iso.cpp")
    exe = str(tmp_path / "vr_shim_iso")
    with open(src, "w") as f:
        f.write(r"""
#include <vr/offscreen_pass_hip.hpp>
#include <cstdio>
int main(int argc, char **)
{
    static_assert(VR_MODE_COMPOSITE == 0 && VR_MODE_MIP == 1 && VR_MODE_ISO == 3, "vr_modes.h");
    if (argc > 1) {  // never taken in the CPU test: needs a device
        Vol::Rendering::Hip::OffscreenPass pass(8, 8);
        pass.render_mode_changed(VR_MODE_ISO);
        pass.isovalue_changed(0.25f);
        return pass.render_mode() == VR_MODE_ISO && pass.isovalue() == 0.25f ? 0 : 1;
    }
    float v = 3.0f;
    std::printf("%d %d %g\n", vr_set_isovalue(nullptr, 0.5f), vr_get_isovalue(nullptr, &v), v);
    return 0;
}
""")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src,
                        "-o", exe, "-L", LIBDIR, "-lvr_amd", "-Wl,-rpath," + LIBDIR],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip() == "-22 -22 3"
