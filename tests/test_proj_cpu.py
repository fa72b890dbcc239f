"""CPU: the minimum- and mean-intensity projection modes (include/vr/vr_modes.h), the
proj_kernel family's names and the reference helper tests/proj_ref.py.

No compute calls (no GPU in the build container): the enum and the binding, argument checks,
the unchanged ABI version and composite code hash, the helper's loop pinned against the C
oracle, the proof that the parity scenes see a wrong order of the mean's additions, the names
resolve_variant yields for modes 4 and 6 against the kernels the library carries, the helper's
closed forms and brick model, and the C++ shim."""
import itertools
import json
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
FULL = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
W, H = 32, 24
CLEAR = np.array([0.11, 0.11, 0.11, 1.0], np.float32)


def scene(camname, box=FULL, tf=None, vol=None, w=W, h=H, vrange=None):
    vol = synth.gaussians_numpy((20, 18, 22), seed=11) if vol is None else vol
    lo, hi = (float(vol.min()), float(vol.max())) if vrange is None else vrange
    return pyoracle.Scene.from_params(vol, lo, hi, synth.tf_color() if tf is None else tf,
                                      synth.camera(camname).to_vr_camera(), w, h,
                                      vr_amd.default_params(), smin=box[0], smax=box[1])


def declared(header):
    src = open(os.path.join(ROOT, "include", "vr", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(vr_[a-z0-9_]+)\s*\(", src))


# ---- 1. the header, the binding ------------------------------------------------------------------
def test_mode_enumerators_and_unchanged_declarations():
    src = open(os.path.join(ROOT, "include", "vr", "vr_modes.h")).read()
    assert re.search(r"VR_MODE_COMPOSITE\s*=\s*0\s*,\s*VR_MODE_MIP\s*=\s*1\s*,\s*VR_MODE_ISO\s*=\s*3", src)
    assert re.search(r"VR_MODE_ISO\s*=\s*3\s*,\s*VR_MODE_MINIP\s*=\s*4\s*,\s*VR_MODE_MEAN\s*=\s*6", src)
    assert (vr_amd.MODE_MINIP, vr_amd.MODE_MEAN) == (4, 6)
    assert (vr_amd.MODE_COMPOSITE, vr_amd.MODE_MIP, vr_amd.MODE_ISO) == (0, 1, 3)
    # no new entry point: both modes are context state set through vr_set_render_mode
    assert declared("vr_modes.h") == {"vr_set_render_mode", "vr_get_render_mode"} == set(vr_amd.MODES_SYMBOLS)
    assert declared("vr_iso.h") == {"vr_set_isovalue", "vr_get_isovalue"} == set(vr_amd.ISO_SYMBOLS)
    assert vr_amd.lib().vr_abi_version() == 9 == vr_amd.ABI_VERSION
    assert "VR_ABI_VERSION 9" in open(os.path.join(ROOT, "include", "vr", "vr.h")).read()
    assert vr_amd.KNOBS["mip_inflight"] == 10


def test_set_render_mode_rejects_null_for_the_new_modes():
    L = vr_amd.lib()
    assert L.vr_set_render_mode(None, 4) == -22
    assert L.vr_set_render_mode(None, 6) == -22


# ---- 2. the helper is pinned by the C oracle, and sees the order ----------------------------------
@pytest.mark.parametrize("camname,box,rays", [("rotA", FULL, 443), ("fill_oblique", SLICE, 698)])
def test_reference_loop_reproduces_the_oracle_composite(camname, box, rays):
    """proj_ref's loop in composite mode is the C oracle bit for bit: same frame, same counters."""
    sc = scene(camname, box)
    ref, st = sc.render()
    got, gs = proj_ref.render(sc, mode="composite")
    assert st["rays"] == rays == gs["rays"]
    assert gs["steps"] == st["steps"] and gs["samples"] == st["samples"]
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    for mode in ("minip", "mean"):  # the same walk whatever is kept (composite ends no ray here)
        img, ms = proj_ref.render(sc, mode=mode)
        assert ms == gs
        assert np.array_equal(np.all(img == CLEAR, axis=-1), np.all(got == CLEAR, axis=-1))


@pytest.mark.parametrize("camname", ["rotA", "fill_oblique"])
def test_parity_scenes_see_the_order_of_the_additions(camname):
    """On the sliced 20x18x22 scenes a mean summed in reverse, or batch by batch, is another
    frame: a kernel that adds in the wrong order cannot pass the parity tests.  A ramp TF, so
    that every change of the mean shows in the pixel."""
    sc = scene(camname, SLICE, tf=synth.tf2())
    ref, _ = proj_ref.render(sc, mode="mean")
    for order in ("reverse", "batch4"):
        other, _ = proj_ref.render(sc, mode="mean", order=order)
        changed = np.any(other.view(np.uint32) != ref.view(np.uint32), axis=-1).sum()
        print(camname, order, "pixels changed:", changed)
        assert changed >= 1
    # the minimum has no order
    mn, _ = proj_ref.render(sc, mode="minip")
    assert not np.array_equal(mn, ref)


# ---- 3. closed forms of the helper ----------------------------------------------------------------
def test_reference_closed_forms():
    """A constant 0.5 volume, slice box inset beyond half a voxel (no sample blends with the
    border): the mean is exactly 0.5 (n additions of 0.5 are exact), the minimum is 0.5, and
    under a one-texel TF (c, a) a pixel with a sample is c a a + clear (1 - a)."""
    vol = np.full((6, 5, 7), 0.5, np.float32)
    tf = np.array([0x80FFFFFF], np.uint32)  # white, alpha 128/255
    box = ((0.2, 0.2, 0.2), (0.8, 0.8, 0.8))
    sc = scene("rotA", box, tf=tf, vol=vol, w=16, h=12, vrange=(0.0, 1.0))
    a = 128.0 / 255.0
    frames = [proj_ref.render(sc, mode=m)[0] for m in ("minip", "mean")]
    assert np.array_equal(frames[0].view(np.uint32), frames[1].view(np.uint32))
    img = frames[0]
    hit = img[..., 3] != 1.0
    assert 0 < hit.sum()
    assert np.allclose(img[hit][:, 3], a * a + 1 - a, rtol=0, atol=1e-6)
    assert np.allclose(img[hit][:, :3], a * a + 0.11 * (1 - a), rtol=0, atol=1e-6)
    assert np.all(img[~hit] == CLEAR)
    # under a ramp the pixel is the TF at 0.5 exactly, in both modes and for every ray length
    ramp = [proj_ref.render(scene("rotA", box, tf=synth.tf2(), vol=vol, w=16, h=12, vrange=(0.0, 1.0)),
                            mode=m)[0] for m in ("minip", "mean")]
    assert np.array_equal(ramp[0].view(np.uint32), ramp[1].view(np.uint32))
    assert len(np.unique(ramp[0][hit].view(np.uint32), axis=0)) == 1
    # the whole cube: entry and exit samples blend with the border 0 and pull the minimum down
    full = proj_ref.render(scene("rotA", FULL, tf=synth.tf2(), vol=vol, w=16, h=12, vrange=(0.0, 1.0)),
                           mode="minip")[0]
    assert not np.array_equal(full, ramp[0])


def test_reference_nan_and_order():
    """A NaN sample leaves the minimum and poisons the mean; _sum's orders are what they say."""
    ds = [np.float32(x) for x in (1e8, 1.0, -1e8, 3.0, 0.25)]
    assert proj_ref._sum(ds, "step") == np.float32(3.25)
    assert proj_ref._sum(ds, "reverse") == np.float32(0.0)
    assert proj_ref._sum(ds, "batch4") == np.float32(3.25)
    vol = np.full((6, 5, 7), 0.5, np.float32)
    vol[3, 2, 3] = np.nan
    sc = scene("rotA", vol=vol, tf=synth.tf2(), w=16, h=12, vrange=(0.0, 1.0))
    mn, _ = proj_ref.render(sc, mode="minip")
    me, _ = proj_ref.render(sc, mode="mean")
    assert np.isfinite(mn).all() and np.isfinite(me).all()  # (a NaN t reads texel 0)
    assert not np.array_equal(mn, me)


def test_brick_model():
    """The model of the stored ranges: 8-cell bricks of padded indices 8 b .. 8 b + 8, the f32
    element's second z on top; NaN bricks are never constant, an infinite constant is not
    skippable, mixed zeros are."""
    assert [proj_ref.brick_grid(n) for n in (40, 36, 44, 20, 13, 7)] == [6, 5, 6, 3, 3, 2]
    g = synth.gaussians_numpy((40, 36, 44), seed=5)
    v = (g / g.max()).astype(np.float32)
    v[v < 0.08] = 0.0
    v = np.minimum(v, np.float32(0.55))
    lo, hi, const = proj_ref.brick_ranges(v)
    assert const.shape == (6, 5, 6) and const.sum() == 50
    assert lo.min() == 0.0 and hi.max() == np.float32(0.55)
    z = np.zeros((20, 20, 20), np.float32)
    z[::2] = -0.0
    assert proj_ref.brick_ranges(z)[2].all()
    z[9, 9, 9] = np.nan  # padded 11: brick 1 on every axis only
    lo, hi, const = proj_ref.brick_ranges(z)
    assert not const[1, 1, 1] and np.isnan(lo[1, 1, 1]) and const.sum() == const.size - 1
    inf = np.full((20, 20, 20), np.inf, np.float32)
    assert not proj_ref.brick_ranges(inf)[2][1, 1, 1]  # an all-inf brick: fetched
    c = proj_ref.brick_ranges(inf[:13, :13, :13])[2]  # padded 2 .. 14: brick 2 holds the border only
    assert c[2, 2, 2] and not c[:2, :2, :2].any()


# ---- 4. variant names for modes 4 and 6 ------------------------------------------------------------
ST_F32, QUAD, ALT, PLAIN, STENCIL, YMAJOR = 4, 0x10, 0x20, 0x100, 0x200, 0x400
BASE_TYPES = {0: "unsigned char", 1: "signed char", 2: "unsigned short", 3: "short", 4: "float",
              0 | QUAD: "vr::Quad8<unsigned char>", 1 | QUAD: "vr::Quad8<signed char>"}
LAYOUTS = list(BASE_TYPES) + [ST_F32 | ALT, ST_F32 | PLAIN, ST_F32 | STENCIL, ST_F32 | YMAJOR]
NS = "void vr::(anonymous namespace)::"
OP = {vr_amd.MODE_MINIP: 0, vr_amd.MODE_MEAN: 1}  # proj_kernel's second template argument


def expected_name(mode, layout, count, skip, k):
    if layout not in BASE_TYPES:
        return None
    if count:
        k = 1
    elif k not in (1, 2, 4):
        return None
    flags = "".join(", true" if f else ", false" for f in (count, skip))
    return f"{NS}proj_kernel<{BASE_TYPES[layout]}, {OP[mode]}{flags}, {k}>(vr::MarchParams, vr::ProjArgs)"


def variant(mode, layout=4, count=0, skip=0, k=2, shade=0):
    return vr_amd.variant_name(layout=layout, mode=mode, shade=shade, count=count, skip=skip, field=0,
                               field_half=0, pipeline=0, tf_n=256, pair=0, mip_inflight=k)


def test_proj_variant_names_are_the_built_kernels():
    reachable = set()
    for mode, layout, count, skip, k, shade in itertools.product(OP, LAYOUTS, (0, 1), (0, 1),
                                                                 (0, 1, 2, 3, 4, 8), (0, 1)):
        got = variant(mode, layout, count, skip, k, shade)
        assert got == expected_name(mode, layout, count, skip, k), (mode, layout, count, skip, k)
        if got is not None:
            reachable.add(got)
    # 7 layouts x {min, mean} x skip x (K = 1, 2, 4 and the counting kernel)
    assert len(reachable) == 7 * 2 * 2 * 4 == 112
    kd = sorted(name[:-3].decode() for name, _ in vr_amd.code_object_symbols()
                if name.endswith(b".kd"))
    dem = subprocess.run(["c++filt"], input="\n".join(kd), capture_output=True, text=True,
                         check=True).stdout.split("\n")
    built = {d for d in dem if "proj_kernel<" in d}
    assert reachable - built == set()
    assert built - reachable == set()
    # the name stays out of the other families' matches, and theirs out of this one's
    for other in ("march_kernel", "march_y_kernel", "march_pair_kernel", "order_tiles_kernel",
                  "mip_kernel", "iso_kernel"):
        assert not any(other in n for n in reachable)
    counts = {fam: sum(f"::{fam}<" in d for d in dem)
              for fam in ("march_kernel", "march_pair_kernel", "mip_kernel", "iso_kernel", "march_y_kernel")}
    assert counts == {"march_kernel": 92, "march_pair_kernel": 32, "mip_kernel": 56, "iso_kernel": 56,
                      "march_y_kernel": 2}
    # 2 and 5 stay unassigned: no projection kernel serves them
    for mode in (2, 5):
        for k in (1, 2, 4):
            assert "proj_kernel" not in (variant(mode, k=k) or "")


def test_composite_code_hash_is_unchanged():
    want = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))["c3"]["code_hash"]
    assert vr_amd.kernel_code_hash() == want


# ---- 5. the shim ------------------------------------------------------------------------------------
def test_shim_compiles_with_the_new_enumerators(tmp_path):
    src = str(tmp_path / "vr_shim_proj.cpp")
    exe = str(tmp_path / "vr_shim_proj")
    with open(src, "w") as f:
        f.write(r"""
#include <vr/offscreen_pass_hip.hpp>
#include <cstdio>
int main(int argc, char **)
{
    static_assert(VR_MODE_COMPOSITE == 0 && VR_MODE_MIP == 1 && VR_MODE_ISO == 3 &&
                      VR_MODE_MINIP == 4 && VR_MODE_MEAN == 6,
                  "vr_modes.h");
    if (argc > 1) {  // never taken in the CPU test: needs a device
        Vol::Rendering::Hip::OffscreenPass pass(8, 8);
        pass.render_mode_changed(VR_MODE_MINIP);
        if (pass.render_mode() != VR_MODE_MINIP) return 1;
        pass.render_mode_changed(VR_MODE_MEAN);
        return pass.render_mode() == VR_MODE_MEAN ? 0 : 1;
    }
    std::printf("%d %d\n", vr_set_render_mode(nullptr, VR_MODE_MINIP),
                vr_set_render_mode(nullptr, VR_MODE_MEAN));
    return 0;
}
""")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src,
                        "-o", exe, "-L", LIBDIR, "-lvr_amd", "-Wl,-rpath," + LIBDIR],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip() == "-22 -22"
