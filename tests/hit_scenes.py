"""Scenes the CPU and GPU tests of the hit records share (test_hit_cpu.py, test_gpu_hit.py,
test_gpu_hit_cli.py) -- test helper.  Volumes, boxes and the frame size: tests/range_scenes.py."""
import numpy as np

import hit_ref
import pyoracle
import synth
import vr_amd
from range_scenes import FULL, H, INSET, SLICE, W, volume

CUT = ((0.45, 0.0, 0.0), (1.0, 1.0, 0.55))
THRESHOLDS = (0.25, 0.9, 1.0)
ISO_F = 0.3  # the isovalue, as a fraction of the data range
KIND = {"entry": vr_amd.HIT_ENTRY, "opacity": vr_amd.HIT_OPACITY, "max": vr_amd.HIT_MAX,
        "min": vr_amd.HIT_MIN, "iso": vr_amd.HIT_ISO}
KEYS = ["entry", "max", "min", "iso"] + [("opacity", float(np.float32(t))) for t in THRESHOLDS]

PARITY = [  # volume, camera, box, TF, W, H
    ("g20", "fill_oblique", FULL, "tfband", W, H),
    ("g20", "rotA", SLICE, "tfc", W, H),
    ("g13", "diag", INSET, "tfband", W, H),
    ("g13", "rotB", FULL, "tfc", W, H),
    ("g20", "fill_oblique", CUT, "tf2", 45, 35),
    ("g20", "near", FULL, "tfc", W, H),
    ("g13", "fill_oblique", FULL, "tfc", 1, 1),
]


def isovalue(v, f=ISO_F):
    lo, hi = float(np.nanmin(v)), float(np.nanmax(v))
    return np.float32(lo + f * (hi - lo))


def key_kind(key):
    """(vr_hit_kind, threshold) of a reference key."""
    return (KIND["opacity"], key[1]) if isinstance(key, tuple) else (KIND[key], 0.5)


def make_scene(volname, camname, box, tfname, w, h, vol=None, vrange=None, tf=None):
    v = np.asarray(volume(volname) if vol is None else vol, dtype=np.float32)
    lo, hi = (float(np.nanmin(v)), float(np.nanmax(v))) if vrange is None else vrange
    return pyoracle.Scene.from_params(v, lo, hi, synth.TFS[tfname]() if tf is None else tf,
                                      synth.camera(camname).to_vr_camera(), w, h,
                                      vr_amd.default_params(), smin=box[0], smax=box[1])


def reference(volname, camname, box, tfname, w=W, h=H, vol=None, vrange=None, iso=None, tf=None,
              thresholds=THRESHOLDS):
    """The hit_ref.Walk of a named scene, computed once per session.  vol / tf: an unnamed volume
    or transfer function, which volname / tfname then only name for the cache."""
    v = np.asarray(volume(volname) if vol is None else vol, dtype=np.float32)
    iso = isovalue(v) if iso is None else np.float32(iso)
    return hit_ref.cached((volname, camname, box, tfname, w, h, vrange),
                          lambda: make_scene(volname, camname, box, tfname, w, h, vol, vrange, tf),
                          iso, thresholds)


def assert_exercised(walk, fourth=False):
    """A parity scene exercises every kind (the reference's own output): at least 30 hits per
    kind and threshold -- 10 at threshold 1.0 of the fourth scene, whose TF is nowhere near
    opaque -- and, for the kinds that can miss a covered pixel, ISO and OPACITY, at least 30
    covered pixels that do.  OPACITY's misses are counted at its two upper thresholds: at 0.25
    the fourth scene has 438 hits among 459 covered pixels, so no bound of 30 holds there."""
    cov = int(walk.covered.sum())
    for key in KEYS:
        hits = int(walk.hits(key).sum())
        low = 10 if fourth and key == ("opacity", 1.0) else 30
        assert hits >= low, (key, hits)
        if key == "iso" or (isinstance(key, tuple) and key[1] >= 0.5):
            assert cov - hits >= 30, (key, cov, hits)
    h = walk.hits("max")
    ms, es = walk.records["max"]["step"][h], walk.records["entry"]["step"][h]
    assert np.unique(ms).size >= 100 and (ms != es).sum() > h.sum() // 2


def words(rec):
    """Hit records as uint32 words, (..., 6): what the tests compare.  A NaN `value` (ENTRY's
    and OPACITY's can be one) compares as one canonical NaN: vr_hit.h leaves its sign and payload
    open, and they differ between the host's and the device's arithmetic -- inf - inf is
    0xFFC00000 on x86 and 0x7FC00000 on the device."""
    rec = np.ascontiguousarray(rec)
    assert rec.dtype == hit_ref.DTYPE and rec.dtype.itemsize == 24
    w = rec.view(np.uint32).reshape(rec.shape + (6,)).copy()
    w[..., 4][np.isnan(rec["value"])] = 0x7FC00000
    return w


def hit_pass(w, h, vol, tf, iso, box=FULL, vrange=None, **knobs):
    rp = vr_amd.OffscreenPass(w, h)
    for k, v in knobs.items():
        rp.set_knob(k, v)
    ds = synth.dataset(np.asarray(vol))
    if vrange is not None:
        ds.vmin, ds.vmax = vrange
    rp.volume_dataset_changed(ds)
    rp.transfer_function_changed(tf)
    rp.slicing_changed(*box)
    rp.isovalue_changed(iso)
    return rp
