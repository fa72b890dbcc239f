"""Scenes the CPU and GPU tests of the mask mesh share (test_mmesh_cpu.py, test_gpu_mmesh.py), the
family's constants read from csrc/vr_mmesh_host.h, and its geometry restated -- test helper.

A scene is (array (bz, by, bx) uint8 or uint32, the volume's dims (nx, ny, nz), origin (x, y, z),
label or None); the volume's own values never enter a mask mesh, only its dims do.
"""
import os
import re

import numpy as np

import mesh_scenes
import mmesh_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_HEADER = os.path.join(ROOT, "volumetric-renderer_amd", "csrc", "vr_mmesh_host.h")


def host_constants():
    """Every `constexpr uint32_t kMmesh... = <integer expression>;` of vr_mmesh_host.h."""
    out = {}
    src = open(HOST_HEADER).read()
    for name, expr in re.findall(r"constexpr uint(?:32|64)_t (kMmesh\w+) = ([^;,]+);", src):
        expr = re.sub(r"\b(0x[0-9A-Fa-f]+|\d+)(?:ull|u)\b", r"\1", expr).replace("/", "//")
        out[name] = int(eval(expr, {"__builtins__": {}}, dict(out)))
    return out


K = host_constants()


def geometry(ext, closed):
    """vr_mmesh_host.h's MmeshGeom of a (bx, by, bz) grid, restated."""
    ring = 1 if closed else 0
    nn = [e + 2 * ring for e in ext]
    nc = [n - 1 for n in nn]
    word = K["kMmeshWord"]
    nw, cw = -(-nn[0] // word), -(-nc[0] // word)
    cell_words = cw * nc[1] * nc[2]
    unit = K["kMmeshScanTile"] * K["kMmeshSpanTiles"]
    groups = max(1, min(K["kMmeshMaxGroups"], -(-cell_words // unit)))
    span = max(unit, -(-(-(-cell_words // groups)) // unit) * unit)
    return dict(nn=nn, nc=nc, nw=nw, cw=cw, node_rows=nn[1] * nn[2], node_words=nn[1] * nn[2] * nw,
                cells=nc[0] * nc[1] * nc[2], cell_words=cell_words, groups=groups, span=span)


def ext_of(a):
    return (a.shape[2], a.shape[1], a.shape[0])


def noise_mask(ext, seed, p=0.5):
    rng = np.random.default_rng(seed)
    return (rng.random((ext[2], ext[1], ext[0])) < p).astype(np.uint8)


def ball():
    """mesh_scenes' small ball at its iso, as a byte mask of the whole 19 x 17 x 21 volume."""
    return (mesh_scenes.small_ball() >= np.float32(0.25)).astype(np.uint8), mesh_scenes.DIMS, (0, 0, 0), None


def noise():
    """mesh_scenes' noise at 0.5: every corner configuration, non-manifold edges, zero normals."""
    m = (mesh_scenes.noise() >= np.float32(0.5)).astype(np.uint8)
    return m, ext_of(m), (0, 0, 0), None


ROW_EXTS = (62, 63, 64, 65, 66)  # closed: 63 .. 67 cells a row; open: 61 .. 65


def row(bx):
    """A grid bx voxels wide: its cell rows end before, at and after the word boundary."""
    m = noise_mask((bx, 5, 4), 100 + bx)
    m[:, :, -2:] = noise_mask((2, 5, 4), 200 + bx, 0.7)  # crossings in the last cells of a row
    return m, (bx, 5, 4), (0, 0, 0), None


THIN_Z = 7000


def thin():
    """3 x 3 x 7000: more node rows than a launch has waves, more cell words than one scan workgroup
    owns, a span of several scan tiles."""
    return noise_mask((3, 3, THIN_Z), 7), (3, 3, THIN_Z), (0, 0, 0), None


INNER_EXT, INNER_ORIGIN = (11, 9, 13), (3, 2, 5)


def inner():
    """A grid inside mesh_scenes' 19 x 17 x 21 volume at a non-zero origin: the ball's middle, cut
    by every face of the grid."""
    full = ball()[0]
    o, e = INNER_ORIGIN, INNER_EXT
    m = np.ascontiguousarray(full[o[2]:o[2] + e[2], o[1]:o[1] + e[1], o[0]:o[0] + e[0]])
    return m, mesh_scenes.DIMS, INNER_ORIGIN, None


LABEL_DIMS = (16, 14, 12)


def labels(label=2):
    """A 4-byte label array of touching blocks 1 .. 6, some voxels 0, one label above 2^31."""
    nx, ny, nz = LABEL_DIMS
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    lab = (1 + x // 6 + 3 * (y // 7)).astype(np.uint32)
    lab[(x + 2 * y + 3 * z) % 7 == 0] = 0
    lab[lab == 5] = 0x80000005
    return lab, LABEL_DIMS, (0, 0, 0), label


def slab(axis):
    """One voxel thick along `axis`: the open form has no cell, the closed form is two cells thick."""
    ext = [7, 6, 5]
    ext[axis] = 1
    return noise_mask(ext, 30 + axis), tuple(ext), (0, 0, 0), None


def zeros():
    return np.zeros((4, 5, 6), np.uint8), (6, 5, 4), (0, 0, 0), None


def ones():
    return np.ones((4, 5, 6), np.uint8), (6, 5, 4), (0, 0, 0), None


SCENES = {"ball": ball, "noise": noise, "thin": thin, "inner": inner, "labels": labels,
          "labels_any": lambda: labels(None), "labels_high": lambda: labels(0x80000005),
          "slab_x": lambda: slab(0), "slab_y": lambda: slab(1), "slab_z": lambda: slab(2),
          "zeros": zeros, "ones": ones}
SCENES.update({"row%d" % bx: (lambda bx=bx: row(bx)) for bx in ROW_EXTS})

_made = {}


def scene(name):
    """The scene, made once (its array is read-only)."""
    if name not in _made:
        a, dims, origin, label = SCENES[name]()
        a.setflags(write=False)
        _made[name] = (a, tuple(dims), tuple(origin), label)
    return _made[name]


def reference(name, closed=True, normals=True, smooth_iters=0, relax=0.5):
    a, dims, origin, label = scene(name)
    return mmesh_ref.cached(name, lambda: (a, dims, origin), label=label, closed=closed, normals=normals,
                            smooth_iters=smooth_iters, relax=relax)
