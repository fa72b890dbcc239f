"""CPU: the hit records (include/vr/vr_hit.h) -- the binding's symbols and structs, the refusals
that need no device, the C++ shim, the host helper header under AddressSanitizer + UBSan in a
stand-alone program (the hit_kernel instantiations: tests/test_kernel_inventory_cpu.py), and the
reference helper tests/hit_ref.py pinned independently: its ISO step and cap mask against
iso_ref, OPACITY against ENTRY and a closed form, MAX's value against proj_ref's MIP pixel.
No GPU: nothing here creates a context."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import hit_ref
import hit_scenes
import iso_ref
import proj_ref
import pyoracle
import synth
import vr_amd
from harness import run_sanitized
from hit_scenes import KEYS, PARITY, THRESHOLDS
from range_scenes import FULL, H, W, volume

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.dirname(vr_amd.LIB_PATH)
F = np.float32


# ---- the binding -------------------------------------------------------------------------------------
def test_every_declared_name_is_exported_and_listed():
    src = open(os.path.join(ROOT, "include", "vr", "vr_hit.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = set(re.findall(r"\b(vr_[a-z0-9_]+)\s*\(", src))
    assert names == set(vr_amd.HIT_SYMBOLS) and len(names) == 4
    out = subprocess.run(["nm", "-D", "--defined-only", vr_amd.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert not names - exported
    L = vr_amd.lib()
    assert all(getattr(L, n).argtypes is not None for n in names)
    assert vr_amd.ABI_VERSION == 9 and L.vr_abi_version() == 9  # an addition: the ABI stays
    assert (vr_amd.HIT_ENTRY, vr_amd.HIT_OPACITY, vr_amd.HIT_MAX, vr_amd.HIT_MIN, vr_amd.HIT_ISO) == (0, 1, 2, 3, 4)
    assert "VR_HIT_ENTRY = 0, VR_HIT_OPACITY = 1, VR_HIT_MAX = 2, VR_HIT_MIN = 3, VR_HIT_ISO = 4" in src
    assert vr_amd.KNOBS["hit_inflight"] == 13 and vr_amd.KNOB_AUTO["hit_inflight"] == -1
    assert "VR_KNOB_HIT_INFLIGHT = 13" in open(os.path.join(ROOT, "include", "vr", "vr_debug.h")).read()
    assert vr_amd.HIT_DTYPE == hit_ref.DTYPE == np.dtype(
        [("pos", "<f4", 3), ("depth", "<f4"), ("value", "<f4"), ("step", "<u4")])
    assert vr_amd.HIT_DTYPE.itemsize == 24


def test_struct_layouts_match_header(tmp_path):
    test = r"""
#include "vr/vr_hit.h"
#include <stdio.h>
#include <stddef.h>
int main(void) { printf("%zu %zu %zu %zu %zu  %zu %zu %zu %zu %zu\n",
  sizeof(vr_hit_request), offsetof(vr_hit_request, kind), offsetof(vr_hit_request, threshold),
  offsetof(vr_hit_request, use_rect), offsetof(vr_hit_request, rect),
  sizeof(vr_hit), offsetof(vr_hit, pos), offsetof(vr_hit, depth), offsetof(vr_hit, value),
  offsetof(vr_hit, step)); return 0; }
"""
    tmp = str(tmp_path / "vr_hit_layout")
    with open(tmp + ".c", "w") as f:
        f.write(test)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), tmp + ".c", "-o", tmp], check=True)
    out = subprocess.run([tmp], capture_output=True, text=True, check=True).stdout.split()
    R, T = vr_amd.vr_hit_request, vr_amd.vr_hit
    assert [int(x) for x in out] == [
        C.sizeof(R), R.kind.offset, R.threshold.offset, R.use_rect.offset, R.rect.offset,
        C.sizeof(T), T.pos.offset, T.depth.offset, T.value.offset, T.step.offset]
    assert C.sizeof(R) == 28 and C.sizeof(T) == 24
    D = vr_amd.HIT_DTYPE
    assert [D.fields[n][1] for n in ("pos", "depth", "value", "step")] == [0, 12, 16, 20]


def test_argument_errors_without_a_device():
    """Everything a NULL context refuses: -22, the outputs untouched."""
    L = vr_amd.lib()
    cam = synth.camera("rotA").to_vr_camera()
    p = vr_amd.default_params()
    req = vr_amd.hit_request(vr_amd.HIT_MAX)
    out = np.full(4, 0x77777777, np.uint32).view(np.uint8)[:24].copy()
    rec = vr_amd.vr_hit()
    rec.step = 77
    st = vr_amd.vr_stats()
    st.rays = 77
    cp, pp, rq = C.byref(cam), C.byref(p), C.byref(req)
    assert L.vr_hit_render(None, cp, pp, rq, out.ctypes.data) == -22
    assert L.vr_hit_render_device(None, cp, pp, rq, out.ctypes.data, None) == -22
    assert L.vr_hit_count_work(None, cp, pp, rq, C.byref(st)) == -22
    assert L.vr_pick(None, cp, pp, rq, 0, 0, C.byref(rec)) == -22
    assert L.vr_hit_render(None, None, None, None, None) == -22
    assert L.vr_pick(None, None, None, None, 0, 0, None) == -22
    assert np.all(out == 0x77) and rec.step == 77 and st.rays == 77
    assert b"NULL" in L.vr_last_error(None)


# ---- the shim ----------------------------------------------------------------------------------------
def test_shim_compiles_with_hit_image_and_pick(tmp_path):
    src = str(tmp_path / "vr_shim_hit.cpp")
    exe = str(tmp_path / "vr_shim_hit")
    with open(src, "w") as f:
        f.write(r"""
#include <vr/offscreen_pass_hip.hpp>
#include <cstdio>
int main(int argc, char **)
{
    static_assert(VR_HIT_ENTRY == 0 && VR_HIT_OPACITY == 1 && VR_HIT_MAX == 2 && VR_HIT_MIN == 3 &&
                      VR_HIT_ISO == 4, "vr_hit.h");
    static_assert(sizeof(vr_hit_request) == 28 && sizeof(vr_hit) == 24, "vr_hit.h");
    if (argc > 1) {  // never taken in the CPU test: needs a device
        Vol::Rendering::Hip::OffscreenPass pass(8, 8);
        Vol::Rendering::Hip::Camera cam{};
        const uint32_t rect[4] = {1, 2, 3, 4};
        const std::vector<vr_hit> img = pass.hit_image(cam, VR_HIT_OPACITY, 0.9f, rect);
        const vr_hit h = pass.pick(cam, 3, 4, VR_HIT_ISO);
        return img.size() == 12 && h.step == 0xFFFFFFFFu ? 0 : 1;
    }
    vr_hit_request req{};
    vr_hit h{};
    vr_stats st{};
    std::printf("%d %d %d %d\n", vr_hit_render(nullptr, nullptr, nullptr, &req, &h),
                vr_hit_render_device(nullptr, nullptr, nullptr, &req, &h, nullptr),
                vr_hit_count_work(nullptr, nullptr, nullptr, &req, &st),
                vr_pick(nullptr, nullptr, nullptr, &req, 0, 0, &h));
    return 0;
}
""")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src,
                        "-o", exe, "-L", LIBDIR, "-lvr_amd", "-Wl,-rpath," + LIBDIR],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip() == "-22 -22 -22 -22"


# ---- the host helper header, stand-alone, under AddressSanitizer + UBSan -----------------------------
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ missing")
def test_host_helpers_under_sanitizers(tmp_path):
    stdout = run_sanitized(tmp_path, "hit")
    seen = 0
    for line in stdout.splitlines():
        w = line.replace(":", " ").split()
        if w[0] != "rect":
            continue
        use, x0, y0, rw, rh = (int(x) for x in w[1:6])
        fw, fh = int(w[7]), int(w[8])
        ok, got = int(w[9]), [int(x) for x in w[10:14]]
        want_ok = use <= 1 and fw > 0 and fh > 0 and (
            not use or (rw >= 1 and rh >= 1 and x0 + rw <= fw and y0 + rh <= fh))
        assert ok == int(want_ok), line
        if ok:
            assert got == ([x0, y0, rw, rh] if use else [0, 0, fw, fh]), line
        seen += 1
    assert seen == 19


# ---- the reference, pinned independently ---------------------------------------------------------------
def test_reference_counts_of_the_parity_scenes():
    """The figures the scenes were chosen by (the reference's own output)."""
    table = {0: (698, 696, 160, 148, 130, 92), 1: (443, 263, 97, 247, 174, 48),
             2: (468, 360, 81, 70, 58, 43), 3: (459, 457, 97, 438, 308, 15)}
    for i, want in table.items():
        w = hit_scenes.reference(*PARITY[i])
        got = (int(w.covered.sum()), int(w.hits("entry").sum()), int(w.hits("iso").sum())) + tuple(
            int(w.hits(("opacity", float(F(t)))).sum()) for t in THRESHOLDS)
        assert got == want, (PARITY[i], got)
        hit_scenes.assert_exercised(w, fourth=i == 3)
        assert np.array_equal(w.hits("max"), w.hits("entry")) and np.array_equal(w.hits("min"), w.hits("entry"))
        # MAX reports a sample of its own: many distinct steps, mostly not the entry's
        h = w.hits("max")
        ms, es = w.records["max"]["step"][h], w.records["entry"]["step"][h]
        assert 120 <= np.unique(ms).size <= 170 and (ms != es).sum() > h.sum() // 2
        # a miss is the miss record exactly, and every record's depth is the f64 distance
        for key in KEYS:
            r = w.records[key]
            miss = ~w.hits(key)
            assert np.array_equal(hit_scenes.words(r[miss]),
                                  hit_scenes.words(hit_ref.miss_records(int(miss.sum()))))
            assert not (w.hits(key) & ~w.covered).any()
            st = w.stats[key]
            assert st["rays"] == int(w.covered.sum()) and st["shaded_samples"] == int(w.hits(key).sum())
            assert st["skipped_samples"] == 0 and st["samples"] <= st["steps"]
        assert w.stats["max"] == w.stats["min"]
        assert w.stats["entry"]["steps"] < w.stats["iso"]["steps"] < w.stats["max"]["steps"]


def test_the_cut_scene_exercises_every_kind_and_the_caps():
    w = hit_scenes.reference(*PARITY[4])
    hit_scenes.assert_exercised(w)
    assert w.cap.sum() >= 10


def test_iso_step_and_cap_equal_iso_ref():
    for volname, camname, box, tfname, w, h in (PARITY[1], PARITY[4]):
        walk = hit_scenes.reference(volname, camname, box, tfname, w, h)
        iso = hit_scenes.isovalue(volume(volname))
        _, st, hit_step, cap = iso_ref.cached(("hit", volname, camname, box, w, h),
                                              lambda: hit_scenes.make_scene(volname, camname, box, "tfc", w, h), iso)
        rec = walk.records["iso"]
        step = np.where(walk.hits("iso"), rec["step"].astype(np.int64), -1)
        assert np.array_equal(step, hit_step) and (hit_step >= 0).sum() >= 30
        assert np.array_equal(walk.cap, cap) and cap.sum() >= 5
        ws = walk.stats["iso"]
        assert (ws["rays"], ws["steps"], ws["samples"]) == (st["rays"], st["steps"], st["samples"])
        # a cap is shown at the sample itself: the entry's position; the refined point of the
        # others lies at or above the isovalue and within one step behind the sample
        ent = walk.records["entry"]
        assert np.array_equal(hit_scenes.words(rec[cap])[:, :3], hit_scenes.words(ent[cap])[:, :3])
        fine = walk.hits("iso") & ~cap
        assert np.all(rec["value"][fine] >= iso) and np.all(rec["depth"][fine] > ent["depth"][fine])


def test_opaque_texel_makes_opacity_one_the_entry():
    """tf0 is one opaque texel: the first in-slab sample brings T to 0, so OPACITY at threshold 1
    is ENTRY in pos and step (and in everything else)."""
    assert synth.tf0().size == 1 and pyoracle.tf_sample(synth.tf0(), 0.3)[3] == 1.0
    w = hit_scenes.reference("g13", "rotB", FULL, "tf0", W, H)
    assert w.hits("entry").sum() >= 30
    for t in THRESHOLDS:
        assert np.array_equal(hit_scenes.words(w.records[("opacity", float(F(t)))]),
                              hit_scenes.words(w.records["entry"]))


@pytest.mark.parametrize("alpha", [0x20, 0x80])
def test_constant_alpha_hits_at_the_closed_form_sample(alpha):
    """A TF of constant alpha a: OPACITY's hit is the n-th in-slab sample of the ray, n the first
    with 1 - (1 - a)^n >= threshold under repeated f32 multiplication."""
    tf = np.full(16, (alpha << 24) | 0x00C08040, np.uint32)
    a = pyoracle.tf_sample(tf, 0.5)[3]
    assert 0.0 < a < 1.0
    w = hit_scenes.reference("g13", "diag", FULL, f"const{alpha}", W, H, tf=tf)
    nth = {}
    for t in THRESHOLDS:
        T, n = F(1.0), 0
        while n < 10000:
            T = T * (F(1.0) - a)
            n += 1
            if F(1.0) - T >= F(t):
                break
        nth[t] = n
    assert nth[0.25] < nth[0.9] < nth[1.0] < 10000
    # the ray's in-slab samples are consecutive steps here (the full box): the n-th is entry + n - 1
    ent = w.records["entry"]
    checked = 0
    for t in THRESHOLDS:
        r = w.records[("opacity", float(F(t)))]
        hit = w.hits(("opacity", float(F(t))))
        assert np.array_equal(r["step"][hit], ent["step"][hit] + np.uint32(nth[t] - 1))
        checked += int(hit.sum())
        assert hit.sum() >= 30 or nth[t] > 100  # (few rays are a hundred samples long)
    assert checked >= 100


def test_max_value_is_the_mip_pixel():
    """MAX's value is the maximum proj_ref puts into the MIP pixel: with a TF whose alpha is 1 and
    whose red rises with the value, the pixel's red is tf(t(value)).r."""
    volname, camname, box, tfname, w, h = PARITY[3]
    walk = hit_scenes.reference(volname, camname, box, tfname, w, h)
    frame, st = proj_ref.cached(("hit", volname, camname, box, tfname, w, h),
                                lambda: hit_scenes.make_scene(volname, camname, box, tfname, w, h), "mip")
    assert (st["rays"], st["steps"], st["samples"]) == tuple(walk.stats["max"][k] for k in ("rays", "steps", "samples"))
    s = hit_scenes.make_scene(volname, camname, box, tfname, w, h).s
    vmin, rng = F(s.vmin), F(s.vmax) - F(s.vmin)
    clear = [F(s.clear[i]) for i in range(4)]
    rec, hit = walk.records["max"], walk.hits("max")
    assert hit.sum() >= 30
    tf = synth.TFS[tfname]()
    one = F(1.0)
    for py, px in zip(*np.nonzero(hit)):
        sc = pyoracle.tf_sample(tf, (rec["value"][py, px] - vmin) / rng)
        T = one * (one - sc[3])
        A = one - T
        omA = one - A
        want = [(sc[c] * sc[3]) * one * A + clear[c] * omA for c in range(3)] + [A * A + clear[3] * omA]
        assert np.array_equal(np.asarray(want, F).view(np.uint32), frame[py, px].view(np.uint32)), (py, px)
    assert np.all(frame[~hit] == np.asarray(clear, F))
    # and the value is the ray's largest sample: no later MIN or ENTRY value exceeds it
    assert np.all(rec["value"][hit] >= walk.records["entry"]["value"][hit])
    assert np.all(rec["value"][hit] >= walk.records["min"]["value"][hit])
