"""Masks for the mask-component tests (tests/test_maskcc_cpu.py, tests/test_gpu_maskcc.py) and their
references from tests/maskcc_ref.py, computed once and shared.  A scene is a (bz, by, bx) uint8
mask of 0/1; shape(name) gives (bx, by, bz).  The scenes are the smallest shapes at which each pass
of the device labelling can go wrong; morph_scenes' masks are reused beside them."""
import functools

import numpy as np

import maskcc_ref
import morph_scenes

ROW_LENGTHS = (1, 63, 64, 65, 129, 257)


def _zeros(bx, by, bz):
    return np.zeros((bz, by, bx), np.uint8)


def _rows(bx):
    """Runs that end at, start at and span the 64-voxel word boundaries, clipped to the row, then
    seeded runs; 4 rows, 2 slices."""
    m = _zeros(bx, 4, 2)
    for b in range(64, bx + 64, 64):
        m[0, 0, max(b - 4, 0):b] = 1       # ends at the boundary
        m[0, 1, b:b + 7] = 1                # starts at it
        m[0, 2, max(b - 2, 0):b + 3] = 1    # spans it
    m[0, 3, :] = 1                          # one run through every word
    rng = np.random.default_rng(900 + bx)
    m[1] = rng.random((4, bx)) < 0.7        # long seeded runs
    return m[:, :, :bx]


def _diag(where):
    """Two runs in neighbouring rows that touch only diagonally across x = 63 | 64."""
    if where == "y":      # rows (j - 1, k) and (j, k)
        m = _zeros(130, 2, 1)
        m[0, 0, 60:64] = 1
        m[0, 1, 64:71] = 1
    elif where == "zy":   # rows (j + 1, k - 1) and (j, k)
        m = _zeros(130, 3, 2)
        m[0, 1, 60:64] = 1
        m[1, 0, 64:67] = 1
    elif where == "yz":   # rows (j - 1, k - 1) and (j, k), the later run on the left
        m = _zeros(130, 3, 2)
        m[0, 0, 64:70] = 1
        m[1, 1, 58:64] = 1
    else:                 # rows (j, k - 1) and (j, k)
        m = _zeros(130, 1, 2)
        m[0, 0, 60:64] = 1
        m[1, 0, 64:66] = 1
    return m


def _random(bx, by, bz, density, seed):
    return (np.random.default_rng(seed).random((bz, by, bx)) < density).astype(np.uint8)


def _corner_pair():
    m = _zeros(2, 2, 2)
    m[0, 0, 0] = m[1, 1, 1] = 1
    return m


def _checker():
    z, y, x = np.meshgrid(np.arange(5), np.arange(9), np.arange(17), indexing="ij", sparse=True)
    return ((x + y + z) % 2 == 0).astype(np.uint8)


def _pillars():
    """Two pillars along y from row 0, in every slice, joined only in the last row of the last slice."""
    m = _zeros(9, 20, 6)
    m[:, :, 1] = m[:, :, 7] = 1
    m[5, 19, 1:8] = 1
    return m


def _comb():
    """40 teeth along y on a spine in the last row."""
    m = _zeros(81, 12, 1)
    m[0, :, 0:80:2] = 1
    m[0, 11, 0:79] = 1
    return m


def _serpentine():
    """One 6-connected chain through 130 x 33 x 4: full rows in x on every second y of every second
    slice, joined at alternating ends, the slices joined by one voxel of the slice between.  The
    root is thousands of steps from the far end."""
    bx, by, bz = 130, 33, 4
    m = _zeros(bx, by, bz)
    at_end = False  # which end of the row the chain stands on
    ys = list(range(0, by, 2))
    for zi, z in enumerate(range(0, bz, 2)):
        rows = ys if zi % 2 == 0 else ys[::-1]
        for i, y in enumerate(rows):
            m[z, y, :] = 1
            at_end = not at_end
            x = bx - 1 if at_end else 0
            if i + 1 < len(rows):
                m[z, (y + rows[i + 1]) // 2, x] = 1
            elif z + 2 < bz:
                m[z + 1, y, x] = 1
    return m


def _spiral():
    """A square spiral, one voxel wide with one voxel between its turns, in 65 x 65 x 1."""
    n = 65
    m = np.zeros((n, n), np.uint8)
    x = y = 0
    dx, dy = 1, 0
    m[0, 0] = 1
    while True:
        moved = False
        while True:
            nx_, ny_ = x + dx, y + dy
            ax, ay = nx_ + dx, ny_ + dy  # the voxel after: the turn ahead must stay clear
            if not (0 <= nx_ < n and 0 <= ny_ < n) or m[ny_, nx_]:
                break
            if 0 <= ax < n and 0 <= ay < n and m[ay, ax]:
                break
            x, y = nx_, ny_
            m[y, x] = 1
            moved = True
        if not moved:
            break
        dx, dy = -dy, dx
    return m.reshape(1, n, n)


def _hole_block(tunnel=False):
    m = _zeros(9, 9, 9)
    m[1:8, 1:8, 1:8] = 1
    m[3:6, 3:6, 3:6] = 0
    if tunnel:
        m[1, 1, 1] = m[2, 2, 2] = 0
    return m


def _cup():
    m = _zeros(9, 9, 9)
    m[1:9, 1:8, 1:8] = 1
    m[3:9, 3:6, 3:6] = 0  # the cavity runs out through the face z = 8
    return m


def _shells():
    m = _zeros(11, 11, 11)
    m[1:10, 1:10, 1:10] = 1
    m[2:9, 2:9, 2:9] = 0
    m[3:8, 3:8, 3:8] = 1
    m[4:7, 4:7, 4:7] = 0
    m[5, 5, 5] = 1
    return m


_MAKERS = {f"row{n}": functools.partial(_rows, n) for n in ROW_LENGTHS}
_MAKERS.update({
    "diag_y": functools.partial(_diag, "y"), "diag_zy": functools.partial(_diag, "zy"),
    "diag_yz": functools.partial(_diag, "yz"), "diag_z": functools.partial(_diag, "z"),
    "line_x": lambda: _random(257, 1, 1, 0.5, 11), "line_y": lambda: _random(1, 300, 1, 0.5, 12),
    "line_z": lambda: _random(1, 1, 257, 0.5, 13),
    "none": lambda: _zeros(129, 5, 3), "all": lambda: _zeros(129, 5, 3) + 1,
    "corner_pair": _corner_pair, "checker": _checker, "pillars": _pillars, "comb": _comb,
    "serpentine": _serpentine, "spiral": _spiral,
    "chunk130": lambda: _random(130, 9, 8, 0.4, 21), "chunk70": lambda: _random(70, 33, 19, 0.4, 22),
    "rand64_05": lambda: _random(64, 64, 64, 0.05, 31), "rand64_50": lambda: _random(64, 64, 64, 0.5, 32),
    "rand64_95": lambda: _random(64, 64, 64, 0.95, 33), "rand128": lambda: _random(128, 96, 80, 0.35, 34),
    "hole_block": _hole_block, "hole_tunnel": functools.partial(_hole_block, True), "cup": _cup, "shells": _shells,
})
OWN = tuple(_MAKERS)
MORPH = tuple(f"morph_{n}" for n in morph_scenes.SHAPES)
NAMES = OWN + MORPH
THIN = ("line_x", "line_y", "line_z", "morph_thin_x", "morph_thin_y", "morph_thin_z")
HOLES = ("hole_block", "hole_tunnel", "cup", "shells")
RANDOM = ("rand64_05", "rand64_50", "rand64_95", "rand128")
# small enough for a breadth-first search in Python
SMALL = tuple(n for n in OWN if n not in RANDOM + ("chunk70",))
# where hole filling is checked: the hole scenes, the random ones, the thin grids and the small scenes
FILL = tuple(dict.fromkeys(HOLES + RANDOM + THIN + SMALL))
# (name, connectivity) -> voxels that hole filling adds
FILLED = {("hole_block", 6): 27, ("hole_block", 26): 27, ("hole_tunnel", 6): 28, ("hole_tunnel", 26): 0,
          ("cup", 6): 0, ("cup", 26): 0}


@functools.lru_cache(maxsize=None)
def mask(name):
    m = morph_scenes.mask(name[6:]) if name.startswith("morph_") else np.ascontiguousarray(_MAKERS[name](), np.uint8)
    assert m.ndim == 3 and m.dtype == np.uint8 and m.max(initial=0) <= 1
    if m.flags.writeable:
        m.setflags(write=False)
    return m


def shape(name):
    return mask(name).shape[::-1]


as_labels = morph_scenes.as_labels


@functools.lru_cache(maxsize=None)
def reference_label(name, connectivity, inverted=False):
    """(labels, records, info) of the scene, or of its complement."""
    m = mask(name) != 0
    labels, rec, info = maskcc_ref.label(~m if inverted else m, connectivity)
    labels.setflags(write=False)
    rec.setflags(write=False)
    return labels, rec, info


@functools.lru_cache(maxsize=None)
def reference_select(name, rule, connectivity=6, min_voxels=0, seed=(0, 0, 0)):
    """(out, info); every rule of a scene shares its one labelling."""
    lab = reference_label(name, connectivity, rule == maskcc_ref.FILL_HOLES)
    out, info = maskcc_ref.select(mask(name), rule, connectivity, min_voxels, seed, labelled=lab)
    out.setflags(write=False)
    return out, info


def last_voxel(name):
    bx, by, bz = shape(name)
    return (bx - 1, by - 1, bz - 1)


def seeds(name):
    """(a set voxel, an unset voxel, the grid's last voxel) as (i, j, k); None where there is none."""
    m = mask(name).reshape(-1)
    bx, by, _ = shape(name)
    at = lambda l: (int(l % bx), int((l // bx) % by), int(l // (bx * by)))
    s, u = np.flatnonzero(m != 0), np.flatnonzero(m == 0)
    return (at(s[s.size // 2]) if s.size else None, at(u[u.size // 2]) if u.size else None, last_voxel(name))
