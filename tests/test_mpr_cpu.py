"""CPU: multi-planar reformat (include/vr/vr_mpr.h) -- the reference helper tests/mpr_ref.py
pinned by closed forms that do not depend on or_trilinear's weights, vr_mpr_axis_plane, the
binding's symbol list and struct, and the conditions the GPU scenes (test_gpu_mpr.py) rely on.
No GPU: nothing here creates a context."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mpr_ref
import synth
import vr_amd
from mpr_scenes import (CF_SHAPE, CLEAR, FULL, OPS, SLICE, closed_form_expected, closed_form_stack,
                        closed_form_volume, face_size, reference)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def ref_plane(pl):
    """The C helper's plane as mpr_ref's dict."""
    return mpr_ref.plane(list(pl.origin), list(pl.du), list(pl.dv), list(pl.dn), pl.width, pl.height,
                         pl.nsamples, pl.op)


# ---- closed forms -----------------------------------------------------------------------------------
@pytest.mark.parametrize("axis,k", [(2, 0), (2, 13), (2, 31), (1, 0), (1, 5), (1, 7), (0, 0), (0, 6), (0, 15)])
def test_thin_axis_slices_show_exactly_one_voxel(axis, k):
    """Image = the face's voxel counts, position = a texel centre: every position is a texel centre,
    every lerp weight 0, the pixel the epilogue of one voxel -- with the stated orientation."""
    vol = closed_form_volume()
    assert vol.shape == CF_SHAPE and len(np.unique(vol)) == vol.size and np.all(np.isfinite(vol))
    lo, hi = float(vol.min()), float(vol.max())
    tf = synth.tf_color()
    w, h = face_size(vol.shape, axis)
    n = vol.shape[2 - axis]
    want = closed_form_expected(vol, axis, k)
    assert want.shape == (h, w)
    for op in OPS.values():
        pl = ref_plane(vr_amd.axis_plane(axis, (k + 0.5) / n, w, h, 1, 0.0, op))
        img, st = mpr_ref.render(vol, lo, hi, tf, pl)
        assert st == dict(rays=w * h, steps=w * h, samples=w * h)
        for py in range(h):
            for px in range(w):
                q = mpr_ref.positions(pl, px, py)[0]
                assert np.array_equal(q * F(vol.shape[::-1]) - F(0.5),
                                      F([(px, py, k), (px, k, vol.shape[0] - 1 - py),
                                         (k, px, vol.shape[0] - 1 - py)][2 - axis]))
                assert np.array_equal(bits(img[py, px]), bits(mpr_ref.pixel_of(want[py, px], lo, hi, tf)))


@pytest.mark.parametrize("axis,k,half", [(2, 13, 2), (1, 4, 1), (0, 8, 3), (2, 1, 1)])
def test_slabs_of_texel_centres_reduce_the_voxel_stack(axis, k, half):
    """spacing = 1 / n and an odd sample count: the samples are the voxels k - half .. k + half,
    so MAX / MIN / MEAN are np.fmax.reduce, np.fmin.reduce and a sequential f32 sum over them."""
    vol = closed_form_volume()
    lo, hi = float(vol.min()), float(vol.max())
    tf = synth.tf_color()
    w, h = face_size(vol.shape, axis)
    n = vol.shape[2 - axis]
    stack = closed_form_stack(vol, axis, k, half)
    ns = 2 * half + 1
    acc = np.zeros((h, w), np.float32)
    for layer in stack:  # in s order
        acc = acc + layer
    want = {"max": np.fmax.reduce(stack), "min": np.fmin.reduce(stack), "mean": acc / F(ns)}
    for opname, op in OPS.items():
        pl = ref_plane(vr_amd.axis_plane(axis, (k + 0.5) / n, w, h, ns, 1.0 / n, op))
        img, st = mpr_ref.render(vol, lo, hi, tf, pl)
        assert st == dict(rays=w * h, steps=w * h * ns, samples=w * h * ns)
        exp = np.array([[mpr_ref.pixel_of(want[opname][py, px], lo, hi, tf) for px in range(w)]
                        for py in range(h)])
        assert np.array_equal(bits(img), bits(exp)), opname
    assert not np.array_equal(want["mean"], want["max"])


def test_mean_order_is_part_of_the_result():
    """The stack's f32 sum in s order differs from the reverse order somewhere: a kernel that adds
    in another order would be told apart by the slab closed form."""
    vol = closed_form_volume()
    stack = closed_form_stack(vol, 0, 8, 3)
    fwd = np.zeros(stack.shape[1:], np.float32)
    rev = np.zeros(stack.shape[1:], np.float32)
    for a, b in zip(stack, stack[::-1]):
        fwd, rev = fwd + a, rev + b
    assert np.any(fwd != rev)


def test_nan_rules_of_the_helper():
    vol = closed_form_volume().copy()
    vol[13, 3, 5] = np.nan
    lo, hi = float(np.nanmin(vol)), float(np.nanmax(vol))
    tf = synth.tf_color()
    imgs = {}
    for opname, op in OPS.items():
        pl = ref_plane(vr_amd.axis_plane(2, 13.5 / 32, 16, 8, 3, 1.0 / 32, op))
        imgs[opname] = mpr_ref.render(vol, lo, hi, tf, pl)[0]
    # the filter's weight-0 lerp fmaf(0, b - a, a) is NaN when the upper neighbour b is: the sample
    # at z = 12 reads the NaN at z + 1 = 13, so of the pixel's three samples only z = 14 is a number
    only = vol[14, 3, 5]
    assert np.array_equal(bits(imgs["max"][3, 5]), bits(mpr_ref.pixel_of(only, lo, hi, tf)))
    assert np.array_equal(bits(imgs["min"][3, 5]), bits(mpr_ref.pixel_of(only, lo, hi, tf)))
    assert np.array_equal(bits(imgs["mean"][3, 5]), bits(mpr_ref.pixel_of(np.nan, lo, hi, tf)))
    # a pixel away from the NaN's footprint: the plain reductions
    col = vol[12:15, 6, 9]
    assert np.array_equal(bits(imgs["max"][6, 9]), bits(mpr_ref.pixel_of(col.max(), lo, hi, tf)))
    assert np.array_equal(bits(imgs["min"][6, 9]), bits(mpr_ref.pixel_of(col.min(), lo, hi, tf)))


# ---- vr_mpr_axis_plane ------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_axis_plane_values(axis):
    w, h, ns = 45, 35, 5
    pl = vr_amd.axis_plane(axis, 0.37, w, h, ns, 0.013, vr_amd.OP_MEAN)
    ref = mpr_ref.axis_plane(axis, 0.37, w, h, ns, 0.013, mpr_ref.OP_MEAN)
    for name in ("origin", "du", "dv", "dn"):
        assert np.array_equal(bits(np.array(list(getattr(pl, name)), F)), bits(ref[name])), name
    assert (pl.width, pl.height, pl.nsamples, pl.op) == (w, h, ns, vr_amd.OP_MEAN)
    origin = [0.5, 0.5, 0.5]
    origin[axis] = 0.37
    assert list(pl.origin) == [float(F(x)) for x in origin]
    ru, rv, sp = float(F(1) / F(w)), float(F(1) / F(h)), float(F(0.013))
    assert list(pl.du) == {2: [ru, 0, 0], 1: [ru, 0, 0], 0: [0, ru, 0]}[axis]
    assert list(pl.dv) == {2: [0, rv, 0], 1: [0, 0, -rv], 0: [0, 0, -rv]}[axis]
    assert list(pl.dn) == [sp if a == axis else 0.0 for a in range(3)]


def test_axis_plane_errors():
    L = vr_amd.lib()
    good = dict(axis=2, position=0.5, width=8, height=8, nsamples=1, spacing=0.01, op=0)

    def call(out=True, **kw):
        a = dict(good, **kw)
        pl = vr_amd.vr_mpr_plane()
        pl.width = 77  # a refused call leaves *out untouched
        rc = L.vr_mpr_axis_plane(a["axis"], a["position"], a["width"], a["height"], a["nsamples"],
                                 a["spacing"], a["op"], C.byref(pl) if out else None)
        assert rc != 0 or pl.width == a["width"]
        assert rc == 0 or pl.width == 77
        return rc

    assert call() == 0
    assert call(nsamples=vr_amd.MPR_MAX_SAMPLES) == 0
    assert call(out=False) == -22
    for bad in (dict(axis=-1), dict(axis=3), dict(position=float("nan")), dict(position=float("inf")),
                dict(spacing=float("nan")), dict(spacing=float("-inf")), dict(width=0), dict(height=0),
                dict(nsamples=0), dict(nsamples=vr_amd.MPR_MAX_SAMPLES + 1), dict(op=3), dict(op=-1)):
        assert call(**bad) == -22, bad
    with pytest.raises(ValueError, match="axis"):
        vr_amd.axis_plane(5, 0.5, 8, 8)
    # the entry points that take a context refuse a NULL one before anything else
    pl, p, st = vr_amd.axis_plane(2, 0.5, 8, 8), vr_amd.default_params(), vr_amd.vr_stats()
    buf = np.zeros((8, 8, 4), np.uint8)
    assert L.vr_mpr_render(None, C.byref(pl), C.byref(p), buf.ctypes.data, 0) == -22
    assert L.vr_mpr_render_device(None, C.byref(pl), C.byref(p), buf.ctypes.data, 0, None) == -22
    assert L.vr_mpr_count_work(None, C.byref(pl), C.byref(p), C.byref(st)) == -22
    assert not buf.any()


# ---- the binding -------------------------------------------------------------------------------------
def test_every_declared_name_is_exported_and_listed():
    src = open(os.path.join(ROOT, "include", "vr", "vr_mpr.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = set(re.findall(r"\b(vr_[a-z0-9_]+)\s*\(", src))
    assert names == set(vr_amd.MPR_SYMBOLS) and len(names) == 4
    out = subprocess.run(["nm", "-D", "--defined-only", vr_amd.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert not names - exported
    L = vr_amd.lib()
    assert all(getattr(L, n).argtypes is not None for n in names)
    assert (vr_amd.OP_MAX, vr_amd.OP_MIN, vr_amd.OP_MEAN) == (0, 1, 2)
    assert "VR_MPR_MAX = 0, VR_MPR_MIN = 1, VR_MPR_MEAN = 2" in src
    assert f"#define VR_MPR_MAX_SAMPLES {vr_amd.MPR_MAX_SAMPLES}" in src


def test_struct_layout_matches_header(tmp_path):
    test = r"""
#include "vr/vr_mpr.h"
#include <stdio.h>
#include <stddef.h>
int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(vr_mpr_plane),
  offsetof(vr_mpr_plane, origin), offsetof(vr_mpr_plane, du), offsetof(vr_mpr_plane, dv),
  offsetof(vr_mpr_plane, dn), offsetof(vr_mpr_plane, width), offsetof(vr_mpr_plane, height),
  offsetof(vr_mpr_plane, nsamples), offsetof(vr_mpr_plane, op)); return 0; }
"""
    tmp = str(tmp_path / "vr_mpr_layout")
    with open(tmp + ".c", "w") as f:
        f.write(test)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), tmp + ".c", "-o", tmp], check=True)
    out = subprocess.run([tmp], capture_output=True, text=True, check=True).stdout.split()
    P = vr_amd.vr_mpr_plane
    assert [int(x) for x in out] == [C.sizeof(P), P.origin.offset, P.du.offset, P.dv.offset, P.dn.offset,
                                     P.width.offset, P.height.offset, P.nsamples.offset, P.op.offset]
    assert C.sizeof(P) == 64


# ---- what the GPU scenes rely on ---------------------------------------------------------------------
def test_gpu_scene_conditions():
    """The oversize oblique plane leaves the cube (some pixels have no step, some have), the SLICE
    box cuts steps off (some steps are no samples), and the slab with its centre plane outside the
    cube still takes samples."""
    w, h = 32, 24
    _, st = reference("g20", "tfc", "oblique", w, h, 5, "mean")
    assert 0 < st["rays"] < w * h
    _, st = reference("g20", "tfc", "oblique", w, h, 5, "mean", pitch=0.02)
    assert st["rays"] == w * h and st["steps"] == st["samples"] == w * h * 5
    _, st = reference("g20", "tf2", 2, w, h, 5, "max", SLICE)
    assert 0 < st["samples"] < st["steps"]
    img, st = reference("g20", "tfc", "outside", 17, 3, 9, "max")
    assert 0 < st["steps"] < 17 * 3 * 9 and st["rays"] == 17 * 3
    assert np.any(img != CLEAR)
