"""Scenes, passes and checks the GPU tests of the range modes share (test_gpu_mip.py,
test_gpu_proj.py; test_gpu_iso.py takes the constants and volumes) -- test helper.

Volumes span three or more bricks per axis with sizes that are no multiple of the brick; the
default frame is no multiple of the 16-pixel tile."""
import numpy as np

import proj_ref
import pyoracle
import synth
import vr_amd

CLEAR = np.array([0.11, 0.11, 0.11, 1.0], np.float32)
SLICE = ((0.2, 0.0, 0.1), (0.8, 1.0, 0.9))
INSET = ((0.06, 0.08, 0.05), (0.94, 0.92, 0.95))  # more than half a voxel of every volume here
FULL = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
W, H = 32, 24
RENDER_MODES = {"mip": vr_amd.MODE_MIP, "minip": vr_amd.MODE_MINIP, "mean": vr_amd.MODE_MEAN}


def plateau():
    g = synth.gaussians_numpy((40, 36, 44), seed=5)
    v = (g / g.max()).astype(np.float32)
    v[v < 0.08] = 0.0
    return np.minimum(v, np.float32(0.55))


VOLUMES = {
    "blob16": lambda: synth.gaussian_blob(16),
    "g20": lambda: synth.gaussians_numpy((20, 18, 22), seed=11),
    "g13": lambda: synth.gaussians_numpy((13, 7, 21), seed=3),
    "plateau": plateau,
}
_vols = {}


def volume(name):
    if name not in _vols:
        v = VOLUMES[name]()
        v.setflags(write=False)
        _vols[name] = v
    return _vols[name]


def int_volume(signed):
    g = volume("g20")
    v = np.rint(g / g.max() * 120.0)
    return (v - 60.0 if signed else v).astype(np.float32)


STORAGE = [  # upload dtype, signed values, knobs, expected storage type (vr::StorageType)
    (np.uint8, False, dict(u8_layout=0), 0), (np.uint8, False, dict(u8_layout=1), 0),
    (np.int8, True, dict(u8_layout=0), 1), (np.int8, True, dict(u8_layout=1), 1),
    (np.uint16, False, {}, 2), (np.int16, True, {}, 3),
    (np.float32, True, dict(narrow=0), 4), (np.float32, True, dict(narrow=1, u8_layout=0), 1),
    (np.int32, False, dict(narrow=1, u8_layout=1), 0), (np.int32, True, dict(narrow=0), 4),
    (np.float64, True, {}, 4),
]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint8)


def mode_pass(mode, w, h, vol, tf, box=FULL, vrange=None, **knobs):
    rp = vr_amd.OffscreenPass(w, h)
    for k, v in knobs.items():
        rp.set_knob(k, v)
    ds = synth.dataset(np.asarray(vol))
    if vrange is not None:
        ds.vmin, ds.vmax = vrange
    rp.volume_dataset_changed(ds)
    rp.transfer_function_changed(tf)
    rp.slicing_changed(*box)
    rp.render_mode_changed(RENDER_MODES[mode])
    assert rp.render_mode == RENDER_MODES[mode]
    return rp


def reference(mode, volname, camname, tfname, box=FULL, w=W, h=H, vol=None, vrange=None):
    """(frame, stats) of proj_ref for a named scene, computed once per session.  The data range
    leaves NaN voxels out (no scene MIP's tests pass here holds one: min / max give the same)."""
    def make():
        v = np.asarray(volume(volname) if vol is None else vol, dtype=np.float32)
        lo, hi = (float(np.nanmin(v)), float(np.nanmax(v))) if vrange is None else vrange
        return pyoracle.Scene.from_params(v, lo, hi, synth.TFS[tfname](), synth.camera(camname).to_vr_camera(),
                                          w, h, vr_amd.default_params(), smin=box[0], smax=box[1])
    return proj_ref.cached((volname, camname, tfname, box, w, h, vrange), make, mode)


def check_against(rp, cam, ref, st, skips=(0, 1)):
    for skip in skips:
        p = vr_amd.default_params(skip_empty=skip)
        img = rp.render(cam, p, vr_amd.OUT_RGBA32F)
        assert np.array_equal(bits(img), bits(ref)), f"skip {skip}: {(bits(img) != bits(ref)).sum()} words differ"
        img8 = rp.render(cam, p, vr_amd.OUT_RGBA8)
        assert np.array_equal(img8, vr_amd.unorm8(ref)), f"skip {skip} (RGBA8)"
        w = rp.count_work(cam, p)
        assert (w["rays"], w["steps"]) == (st["rays"], st["steps"]), (skip, w, st)
        assert w["samples"] + w["skipped_samples"] == st["samples"], (skip, w, st)
        assert w["shaded_samples"] == 0
        if not skip:
            assert w["skipped_samples"] == 0


def skip_pair(rp, cam, fmt=vr_amd.OUT_RGBA32F):
    """skip_empty 0 against 1: the same bits and in-slab samples; returns the frame and the
    skipping pass's counters."""
    a = rp.render(cam, vr_amd.default_params(skip_empty=0), fmt)
    b = rp.render(cam, vr_amd.default_params(skip_empty=1), fmt)
    assert np.array_equal(bits(a), bits(b))
    w0 = rp.count_work(cam, vr_amd.default_params(skip_empty=0))
    w1 = rp.count_work(cam, vr_amd.default_params(skip_empty=1))
    assert w0["skipped_samples"] == 0 and (w0["rays"], w0["steps"]) == (w1["rays"], w1["steps"])
    assert w1["samples"] + w1["skipped_samples"] == w0["samples"]
    assert w0["shaded_samples"] == 0 == w1["shaded_samples"]
    return a, w1
