"""Scenes the MPR tests share (test_mpr_cpu.py, test_gpu_mpr.py) -- test helper.

Volumes, boxes and the clear colour are those of tests/range_scenes.py (three or more bricks per
axis, sizes that are no brick multiple).  References come from tests/mpr_ref.py, one per scene
and session."""
import numpy as np

import mpr_ref
import synth
from range_scenes import CLEAR, FULL, INSET, SLICE, volume  # noqa: F401

OPS = {"max": mpr_ref.OP_MAX, "min": mpr_ref.OP_MIN, "mean": mpr_ref.OP_MEAN}
POSITION = 0.37
SPACING = 0.013
PITCH_OVER, PITCH_IN = 0.05, 0.02  # the oblique image overhangs the cube / lies inside it

# The closed-form volume: power-of-two sizes, distinct finite values (no two voxels equal, none 0).
CF_SHAPE = (32, 8, 16)  # nz, ny, nx


def closed_form_volume():
    nz, ny, nx = CF_SHAPE
    rng = np.random.default_rng(7)
    # (full mantissas: the f32 sum of a few of them rounds, so its order shows)
    v = (rng.permutation(nz * ny * nx).astype(np.float32) + np.float32(1.0)) * np.float32(0.0137)
    return v.reshape(nz, ny, nx)


def closed_form_expected(vol, axis, k):
    """(H, W) voxels an axis slice at texel centre k shows, with the stated orientation."""
    nz = vol.shape[0]
    if axis == 2:
        return vol[k]                    # [py, px]
    if axis == 1:
        return vol[::-1, k, :]           # vol[nz-1-py, k, px]
    assert nz == vol.shape[0]
    return vol[::-1, :, k]               # vol[nz-1-py, px, k]


def closed_form_stack(vol, axis, k, half):
    """(2 half + 1, H, W): the voxels of the slab's samples s = 0 .. 2 half, in s order."""
    return np.stack([closed_form_expected(vol, axis, k + j) for j in range(-half, half + 1)])


def face_size(shape, axis):
    """(width, height) in voxels of the face an axis plane shows."""
    nz, ny, nx = shape
    return {2: (nx, ny), 1: (nx, nz), 0: (ny, nz)}[axis]


def make_plane(kind, w, h, nsamples, op, pitch=PITCH_OVER):
    """kind: 0, 1, 2 (axis planes at POSITION), "oblique", or "outside" (an axial slab whose
    centre plane lies above the cube while its lower samples lie inside)."""
    if kind == "oblique":
        return mpr_ref.oblique_plane(pitch, w, h, nsamples, op, SPACING)
    if kind == "outside":
        return mpr_ref.axis_plane(2, 1.03, w, h, nsamples, SPACING, op)
    return mpr_ref.axis_plane(kind, POSITION, w, h, nsamples, SPACING, op)


def reference(volname, tfname, kind, w, h, nsamples, opname, box=FULL, pitch=PITCH_OVER, vol=None):
    def make():
        v = np.asarray(volume(volname) if vol is None else vol, dtype=np.float32)
        lo, hi = float(np.nanmin(v)), float(np.nanmax(v))
        return mpr_ref.render(v, lo, hi, synth.TFS[tfname](), make_plane(kind, w, h, nsamples, OPS[opname], pitch),
                              box, CLEAR)
    return mpr_ref.cached((volname, tfname, kind, w, h, nsamples, opname, box, pitch), make)
