"""Scenes the CPU and GPU tests of connected-component labelling share (test_label_cpu.py,
test_gpu_label.py), each with the reference's own counts pinned beside it -- test helper."""
import numpy as np

import label_ref
import mesh_scenes

F = np.float32
INF = float("inf")
DIMS = mesh_scenes.DIMS  # 19 x 17 x 21: three bricks per axis, no multiple of a brick
BOX = mesh_scenes.BOX    # interior, not brick-aligned
LONG_BOX = ((2, 3, 100), (22, 20, 2900))


def noise():
    """21 x 17 x 19 (z, y, x) uniform noise: hundreds of small components, many across bricks."""
    return np.random.default_rng(7).random((21, 17, 19), dtype=F)


def snake():
    """One 6-connected path through all of 19 x 17 x 21: rows in x on every second y and z, joined
    at alternating ends.  Its root is thousands of path steps from its far end."""
    nx, ny, nz = DIMS
    v = np.zeros((nz, ny, nx), F)
    x_at_end = False  # which end of the row the path stands on
    ys = list(range(0, ny, 2))
    for zi, z in enumerate(range(0, nz, 2)):
        rows = ys if zi % 2 == 0 else ys[::-1]
        for ri, y in enumerate(rows):
            v[z, y, :] = 1.0
            x_at_end = not x_at_end
            x = nx - 1 if x_at_end else 0
            if ri + 1 < len(rows):
                v[z, (y + rows[ri + 1]) // 2, x] = 1.0
            elif z + 2 < nz:
                v[z + 1, y, x] = 1.0
    return v


def checker(dims=DIMS, dtype=F):
    """(x + y + z) even: the most components a volume can hold under 6, one under 26."""
    nx, ny, nz = dims
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij", sparse=True)
    return ((x + y + z) % 2 == 0).astype(dtype)


def long_checker():
    return checker((24, 24, 3000), np.uint8)


# name -> volume maker
SCENES = {
    "noise": noise,
    "snake": snake,
    "checker": checker,
    "ball": mesh_scenes.small_ball,
    "bigball": mesh_scenes.big_ball,
    "integers": mesh_scenes.integers,
    "specials": mesh_scenes.specials,
    "long_thin": mesh_scenes.long_thin,
    "long_checker": long_checker,
}
# noise under 6: [0.7, 1] has 448 components, 43 of at least 10 voxels, 62 across a brick boundary.
# The 26-connected window of `noise`, chosen by the reference: 140 components, 28 across a brick
# boundary (at 0.88 one component of 563 voxels swallows most of them).
NOISE26 = (0.9, 1.0)
STRADDLE = {("noise", 0.7, 1.0, 6): 62, ("noise", 0.3, 0.6, 6): 74, ("noise", 0.9, 1.0, 26): 28}

# (scene, lo, hi, connectivity, box) -> the reference's pinned
# (components, in_voxels, largest_voxels, largest_label)
CASES = {
    ("noise", 0.7, 1.0, 6, None): (448, 2082, 213, 138),
    ("noise", 0.7, 1.0, 6, BOX): (141, 515, 117, 665),
    ("noise", 0.3, 0.6, 6, None): (447, 2017, 167, 708),
    ("noise", 0.3, 0.6, 6, BOX): (143, 493, 57, 681),
    ("noise", 0.9, 1.0, 26, None): (140, 654, 93, 656),
    ("noise", 0.9, 1.0, 26, BOX): (42, 161, 35, 39),
    ("snake", 0.5, 1.0, 6, None): (1, 1979, 1979, 1),
    ("snake", 0.5, 1.0, 6, BOX): (36, 432, 12, 133),
    ("snake", 0.5, 1.0, 26, None): (1, 1979, 1979, 1),
    ("snake", 0.5, 1.0, 26, BOX): (36, 432, 12, 133),
    ("checker", 0.5, 1.0, 6, None): (3392, 3392, 1, 1),
    ("checker", 0.5, 1.0, 6, BOX): (858, 858, 1, 1),
    ("checker", 0.5, 1.0, 26, None): (1, 3392, 3392, 1),
    ("checker", 0.5, 1.0, 26, BOX): (1, 858, 858, 1),
    ("ball", 0.25, INF, 6, None): (1, 792, 792, 1737),
    ("ball", 0.25, INF, 6, BOX): (1, 779, 779, 53),
    ("ball", 0.25, INF, 26, None): (1, 792, 792, 1737),
    ("ball", 0.25, INF, 26, BOX): (1, 779, 779, 53),
    ("bigball", 20.25, INF, 6, None): (1, 5593, 5593, 46),
    ("bigball", 20.25, INF, 6, BOX): (1, 1716, 1716, 1),
    ("bigball", 20.25, INF, 26, None): (1, 5593, 5593, 46),
    ("bigball", 20.25, INF, 26, BOX): (1, 1716, 1716, 1),
    ("specials", -INF, INF, 6, None): (1, 6763, 6763, 1),
    ("specials", -INF, INF, 6, BOX): (1, 1709, 1709, 1),
    ("specials", -INF, INF, 26, None): (1, 6763, 6763, 1),
    ("specials", -INF, INF, 26, BOX): (1, 1709, 1709, 1),
    ("specials", 0.25, INF, 6, None): (20, 805, 786, 1737),
    ("specials", 0.25, INF, 6, BOX): (3, 775, 773, 53),
    ("specials", 0.25, INF, 26, None): (17, 805, 788, 1737),
    ("specials", 0.25, INF, 26, BOX): (2, 775, 774, 53),
}
# the scenes of 24 x 24 x 3000: more bricks than a launch has workgroups, more chunks than one
# round of the table's scan
LONG_CASES = {
    ("long_thin", 128.0, 255.0, 6, None): (1, 164005, 164005, 323),
    ("long_thin", 128.0, 255.0, 6, LONG_BOX): (1, 147767, 147767, 71),
    ("long_thin", 128.0, 255.0, 26, None): (1, 164005, 164005, 323),
    ("long_thin", 128.0, 255.0, 26, LONG_BOX): (1, 147767, 147767, 71),
    ("long_thin", 0.0, 127.0, 6, None): (1, 1563995, 1563995, 1),
    ("long_thin", 0.0, 127.0, 6, LONG_BOX): (1, 804233, 804233, 1),
    ("long_thin", 0.0, 127.0, 26, None): (1, 1563995, 1563995, 1),
    ("long_thin", 0.0, 127.0, 26, LONG_BOX): (1, 804233, 804233, 1),
    ("long_checker", 1.0, 1.0, 6, None): (864000, 864000, 1, 1),
    ("long_checker", 1.0, 1.0, 6, LONG_BOX): (476000, 476000, 1, 2),
    ("long_checker", 1.0, 1.0, 26, None): (1, 864000, 864000, 1),
    ("long_checker", 1.0, 1.0, 26, LONG_BOX): (1, 476000, 476000, 2),
    ("long_checker", 0.0, 0.0, 6, None): (864000, 864000, 1, 2),
    ("long_checker", 0.0, 0.0, 6, LONG_BOX): (476000, 476000, 1, 1),
    ("long_checker", 0.0, 0.0, 26, None): (1, 864000, 864000, 2),
    ("long_checker", 0.0, 0.0, 26, LONG_BOX): (1, 476000, 476000, 1),
}


def reference(name, lo, hi, connectivity=6, box=None):
    """(labels, records, info) of label_ref, computed once per session."""
    return label_ref.cached(name, SCENES[name], lo, hi, connectivity, box)


def pinned(info):
    return (info["components"], info["in_voxels"], info["largest_voxels"], info["largest_label"])


def straddling(labels, origin=(0, 0, 0), cells=(8, 8, 8), pad=2):
    """How many components have voxels in more than one brick (bricks of `cells` cells on the
    padded index = volume index + pad)."""
    lab = labels.reshape(-1)
    sel = np.flatnonzero(lab)
    if not sel.size:  # no component: reduceat refuses an empty array
        return 0
    nz, ny, nx = labels.shape
    bx = (sel % nx + origin[0] + pad) // cells[0]
    by = ((sel // nx) % ny + origin[1] + pad) // cells[1]
    bz = (sel // (nx * ny) + origin[2] + pad) // cells[2]
    brick = bx + 4096 * (by + 4096 * bz)
    order = np.argsort(lab[sel], kind="stable")
    ls, bs = lab[sel][order], brick[order]
    starts = np.flatnonzero(np.r_[True, ls[1:] != ls[:-1]])
    return int(np.count_nonzero(np.minimum.reduceat(bs, starts) != np.maximum.reduceat(bs, starts)))
