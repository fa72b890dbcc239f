"""Scenes the CPU and GPU tests of include/vr/vr_mview.h share (test_mview_cpu.py, test_gpu_mview.py)
-- test helper.  Cameras, boxes and frame sizes are hit_scenes' and edge_shapes'; what is added here:
the arrays laid over those volumes, the grid that lies inside its volume with a cut cell on every
axis, and the open slice box, under which a ray that enters through a far face takes an in-slab
sample at exactly 1.0, whose voxel index is clamped."""
import numpy as np

import hit_scenes
import mstat_scenes
import mview_ref as R
import synth
import vr_amd
from range_scenes import FULL, INSET, SLICE, volume

F = np.float32
OPEN = ((-1.0, -1.0, -1.0), (2.0, 2.0, 2.0))  # every position of the walk is in-slab, 1.0 included

# ---- the grid inside a volume ---------------------------------------------------------------------------
GRID_VOLUME = (43, 24, 20)  # (nx, ny, nz)
GRID_EXT = (37, 19, 17)     # 5 x 3 x 3 = 45 cells: two words, a cell row across the word boundary,
GRID_ORIGIN = (5, 3, 2)     # a cut cell on every axis; the origin is no multiple of 8
BIG_DIMS = mstat_scenes.BIG_DIMS  # 130 x 70 x 33: 17 x 9 x 5 cells, 24 words: more than one workgroup
THIN_GRIDS = ((1, 19, 17), (37, 1, 17), (37, 19, 1))
WORD_VALUES = (2, 256, 65536, 0x01000000, 0xFFFFFFFF)
DENSITIES = (0.02, 0.5)
STEPS = (0.005, None)  # None: 1 / max(dims)


def shape_of(ext):
    return tuple(ext[::-1])


def grid_volume():
    return synth.gaussians_numpy(GRID_VOLUME, seed=17)


def byte_mask(ext, density, seed=0):
    return mstat_scenes.byte_mask(shape_of(ext), density, seed)


def word_mask(ext, seed=0):
    return mstat_scenes.word_mask(shape_of(ext), seed)


def blob_mask(volname, f=0.3):
    """The voxels of a named volume above f of its maximum, with a sprinkle of specks around them:
    surfaces to hit, empty space to miss in, and cells that are set where the ray's voxel is not."""
    v = volume(volname)
    m = v > F(f) * v.max()
    m |= mstat_scenes.byte_mask(v.shape, 0.004, 5) != 0
    return m.astype(np.uint8)


def corner_voxel(ext):
    """A single set voxel, in the (7, 7, 7) corner of cell (0, 0, 0)."""
    m = np.zeros(shape_of(ext), np.uint8)
    m[7, 7, 7] = 1
    return m


def at_odd_address(a):
    """A copy of the bytes of `a` that starts at an odd address (host memory)."""
    buf = np.zeros(a.nbytes + 16, np.uint8)
    off = 1 if buf.ctypes.data % 2 == 0 else 0
    out = buf[off:off + a.nbytes]
    out[:] = a.reshape(-1).view(np.uint8)
    assert out.ctypes.data % 2 == 1
    return out


def params(dims, step):
    return vr_amd.default_params(step=float(F(1.0) / F(max(dims))) if step is None else step)


def parity_scene(i, step=0.005, box=None):
    """hit_scenes.PARITY[i] as a pyoracle.Scene with this step (and box, where given)."""
    volname, camname, b, tfname, w, h = hit_scenes.PARITY[i]
    s = hit_scenes.make_scene(volname, camname, b if box is None else box, tfname, w, h)
    s.s.step = float(F(1.0) / F(max(volume(volname).shape))) if step is None else step
    return s


def parity_reference(i, step=0.005, box=None):
    """(records, info, trace) of the blob mask over parity scene i, once per session."""
    volname = hit_scenes.PARITY[i][0]
    return R.cached(("parity", i, step, box), lambda: R.hit_image(parity_scene(i, step, box), blob_mask(volname)))


def grid_scene(camname, box, w, h, step=0.005):
    import pyoracle
    v = grid_volume()
    p = params(GRID_VOLUME, step)
    return pyoracle.Scene.from_params(v, float(v.min()), float(v.max()), synth.tf_color(),
                                      synth.camera(camname).to_vr_camera(), w, h, p, smin=box[0], smax=box[1])


def face_cells(ext, index):
    """For box-linear indices of the grid: per axis and side, whether the voxel lies in the first
    cell layer / the last (cut) cell layer of that axis."""
    idx = np.asarray(index, np.int64)
    g = [idx % ext[0], idx // ext[0] % ext[1], idx // (ext[0] * ext[1])]
    return {(a, side): (g[a] // R.CELL == (0 if side == 0 else (ext[a] - 1) // R.CELL)) for a in range(3) for side in (0, 1)}
