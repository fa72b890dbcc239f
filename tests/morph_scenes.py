"""Masks for the distance-transform and morphology tests (tests/test_morph_cpu.py, tests/
test_gpu_morph.py), and their references from tests/morph_ref.py, computed once and shared.
A scene is a (bz, by, bx) uint8 mask of 0/1; SHAPES gives (bx, by, bz)."""
import functools

import numpy as np

import morph_ref

SHAPES = {
    "sparse70": (70, 33, 19),     # density 0.01: odd extents, more than one word a row, several tiles
    "rows129": (129, 5, 3),       # density 0.5: rows longer than two waves
    "thin_x": (257, 1, 1),        # about 3 set voxels
    "thin_y": (1, 300, 1),
    "thin_z": (1, 1, 257),
    "dense64": (64, 64, 64),      # density 0.999
    "sparse64": (64, 64, 64),     # density 0.001
    "far200": (200, 160, 96),     # about 30 set voxels: long searches, distances into the thousands
    "corner": (70, 33, 19),       # one set voxel, at the origin
    "empty": (129, 5, 3),
    "full": (129, 5, 3),
    "long_y": (3, 16400, 1),      # a column of more than 16384 voxels: the long-column axis kernel
}
SMALL = ("sparse70", "rows129", "thin_x", "thin_y", "thin_z", "corner", "empty", "full")  # every r2
BIG = ("dense64", "sparse64", "far200", "long_y")
R2 = (0, 1, 2, 3, 9, 100)


def diagonal2(name):
    bx, by, bz = SHAPES[name]
    return (bx - 1) ** 2 + (by - 1) ** 2 + (bz - 1) ** 2


@functools.lru_cache(maxsize=None)
def mask(name):
    bx, by, bz = SHAPES[name]
    rng = np.random.default_rng(sorted(SHAPES).index(name) + 4100)
    n = bx * by * bz
    m = np.zeros(n, np.uint8)
    density = {"sparse70": 0.01, "rows129": 0.5, "dense64": 0.999, "sparse64": 0.001}
    count = {"thin_x": 3, "thin_y": 3, "thin_z": 3, "far200": 30, "long_y": 12}
    if name in density:
        m[rng.random(n) < density[name]] = 1
    elif name in count:
        m[rng.choice(n, count[name], replace=False)] = 1
    elif name == "corner":
        m[0] = 1
    elif name == "full":
        m[:] = 1
    m = m.reshape(bz, by, bx)
    m.setflags(write=False)
    return m


def as_labels(m):
    """The same set as a 4-byte mask: label-like values, some with a zero low byte."""
    idx = np.arange(m.size, dtype=np.uint32).reshape(m.shape)
    return np.where(m != 0, (idx + 1) << 8, 0).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def reference_edt(name, target):
    d, info = morph_ref.edt(mask(name), target)
    d.setflags(write=False)
    return d, info


@functools.lru_cache(maxsize=None)
def _dist(name, target):
    return reference_edt(name, target)[0]


@functools.lru_cache(maxsize=None)
def reference_morph(name, op, r2):
    """(out uint8, info); dilations and erosions of a scene share its two transforms."""
    m = mask(name) != 0
    if op == morph_ref.DILATE:
        out = _dist(name, morph_ref.TO_SET) <= r2
    elif op == morph_ref.ERODE:
        out = _dist(name, morph_ref.TO_UNSET) > r2
    elif op == morph_ref.OPEN:
        out = morph_ref.dilate(reference_morph(name, morph_ref.ERODE, r2)[0] != 0, r2)
    else:
        out = morph_ref.erode(reference_morph(name, morph_ref.DILATE, r2)[0] != 0, r2)
    out = out.astype(np.uint8)
    out.setflags(write=False)
    return out, {"voxels": int(m.size), "in_set": int(m.sum()), "out_set": int(out.sum())}


def morph_cases():
    """(name, op, r2): every op and r2 (and one above the diagonal) on the small scenes; on the big
    ones r2 = 9 for every op and 100 for dilation and erosion, which cost no further transform."""
    cases = []
    for name in SMALL:
        for r2 in R2 + (diagonal2(name) + 1,):
            cases += [(name, op, r2) for op in range(4)]
    for name in BIG:
        cases += [(name, op, 9) for op in range(4)]
        cases += [(name, op, 100) for op in (morph_ref.DILATE, morph_ref.ERODE)]
    return cases
