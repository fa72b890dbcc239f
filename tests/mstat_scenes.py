"""Scenes the CPU and GPU tests of include/vr/vr_mstat.h share (test_mstat_cpu.py, test_gpu_mstat.py)
-- test helper.  The volumes and boxes are edge_shapes' and label_scenes'; what is added here: the
two signed layouts, the arrays laid over a volume (a 1-byte mask, a 4-byte mask whose elements are
at least 2), a volume of special values with a label array that gives each of them a region of its
own, the volume that takes more than one workgroup, and the thin grid that has more tiles than a launch
has workgroups."""
import numpy as np

import edge_shapes as E
import label_ref
import label_scenes

F = np.float32
INF = float("inf")

# name -> upload dtype, knobs, vr::StorageType, the kernels' tag, what is added to edge_shapes' fill
LAYOUTS = {
    "f32": (np.float32, dict(narrow=0), 4, "f32", 0),
    "u16": (np.uint16, {}, 2, "u16", 0),
    "i16": (np.int16, {}, 3, "i16", -50),
    "quad8": (np.uint8, dict(u8_layout=1), 0, "quad_u8", 0),
    "plain8": (np.uint8, dict(u8_layout=0), 0, "u8", 0),
    "i8": (np.int8, dict(u8_layout=1), 1, "quad_i8", -50),
    "i8plain": (np.int8, dict(u8_layout=0), 1, "i8", -50),
}
HIST = (16, 10.0, 80.0)    # of the fill 0 .. 100: voxels below, above and on hi
WINDOW = (20.0, 50.0)      # edge_shapes' second window: the upper bound is a stored value


def volume(dims, layout):
    """(nz, ny, nx) f32 of integers, as `layout` stores them."""
    return E.fill(dims, "noise") + F(LAYOUTS[layout][4])


def shifted(layout, *values):
    return tuple(v + LAYOUTS[layout][4] for v in values)


def byte_mask(shape, density=0.5, seed=0):
    bz, by, bx = shape
    rng = np.random.default_rng(1000 + bx + 100 * by + 10000 * bz + seed)
    return (rng.random(shape) < density).astype(np.uint8)


def word_mask(shape, seed=0):
    """uint32, set elements at least 2 (nothing may read one byte of it, or compare it with 1)."""
    m = byte_mask(shape, 0.6, seed + 1).astype(np.uint32)
    rng = np.random.default_rng(7 + seed)
    return m * rng.choice(np.array([2, 256, 65536, 0x01000000, 0xFFFFFFFF], np.uint32), shape)


# ---- special values -------------------------------------------------------------------------------------
SPECIAL_DIMS = (13, 6, 5)  # (nx, ny, nz): two bricks in x of either geometry
DENORMAL = F(1e-45)
SPECIAL_TABLE = (3, 7, 8, 20, 21, 30, 40, 45, 50, 60)  # 8: an empty region; label 99 is in no table
UNLISTED = 99


def specials():
    """(volume, labels): f32 noise in (-1, 1) with NaN, +-inf, -0.0 and a denormal, and a label array
    (rows of x, a label per row) that gives each of them a region:
       3  plain noise                       7  noise with two NaNs
      20  all NaN                           21  +inf and -inf: the sums are NaN
      30  +inf alone above noise            40  -0.0 before +0.0, nothing else: both extremes zero, at the -0.0
      45  -0.0 twice and nothing else: the sums are +0.0
      50  its maximum twice, its minimum twice: the smaller index wins
      60  zeros and a denormal: the denormal is the maximum and the only non-zero term
      99  not in the table"""
    nx, ny, nz = SPECIAL_DIMS
    rng = np.random.default_rng(11)
    v = (rng.random((nz, ny, nx), dtype=F) * F(2.0) - F(1.0)) * F(0.9)
    lab = np.zeros((nz, ny, nx), np.uint32)
    lab[0, 0, :], lab[0, 1, 2:], lab[0, 3, :], lab[1, 0, 1:12] = 3, 7, 20, 21
    lab[1, 2, :], lab[2, 1, 3:9], lab[2, 3, :], lab[3, 0, :], lab[4, 5, 4:] = 30, 40, 50, 60, UNLISTED
    lab[3, 4, 0:3] = 3  # (a region in two pieces)
    lab[4, 0, 0:2] = 45
    v[4, 0, 0:2] = -0.0
    v[0, 1, 5] = v[0, 1, 12] = np.nan
    v[0, 3, :] = np.nan
    v[1, 0, 3], v[1, 0, 9] = np.inf, -np.inf
    v[1, 2, 6] = np.inf
    v[2, 1, 3:9] = 0.0
    v[2, 1, 3] = -0.0
    v[2, 3, 4] = v[2, 3, 10] = 0.95
    v[2, 3, 2] = v[2, 3, 7] = -0.95
    v[3, 0, :] = 0.0
    v[3, 0, 8] = DENORMAL
    v.setflags(write=False)
    lab.setflags(write=False)
    return v, lab


# ---- beyond one workgroup -------------------------------------------------------------------------------
BIG_DIMS = (130, 70, 33)  # 3 x 18 x 33 tiles of 64 x 4: more than a workgroup, rows that end inside a tile
BIG_DENSITIES = (0.05, 0.5, 0.95)
_big = {}


def big_volume(layout):
    """u16: every code 0 .. 65535 (sum2 beyond 2^48: no 32-bit partial sum holds it); f32: normal deviates, hardly one an integer."""
    if layout not in _big:
        nx, ny, nz = BIG_DIMS
        rng = np.random.default_rng(23)
        if layout == "u16":
            v = rng.integers(0, 65536, (nz, ny, nx)).astype(F)
        else:
            v = (rng.standard_normal((nz, ny, nx)) * 1000.0).astype(F)
        v.setflags(write=False)
        _big[layout] = v
    return _big[layout]


def checker_labels(dims=BIG_DIMS):
    """The labels of the checker under 6-connectivity: every set voxel its own component, 1 + its index."""
    c = label_scenes.checker(dims, np.uint8)
    idx = np.arange(c.size, dtype=np.uint32).reshape(c.shape)
    return np.where(c != 0, idx + np.uint32(1), np.uint32(0)).astype(np.uint32)


# ---- more tiles than workgroups -------------------------------------------------------------------------
# A voxel pass launches at most 4096 workgroups and strides: only a grid of more than 4096 tiles makes a
# workgroup walk a second tile, a lane gather more than one voxel, and a lane of the label pass arrive
# with sums it already keeps.  70 x 5 x 9000 is 2 x 2 x 9000 = 36 000 tiles of 64 x 4 (8 or 9 a
# workgroup, 1024 slices apart) in 3.15 M voxels, a box at (1, 1, 1) of a volume one voxel larger all
# round.
MAX_GRID = 4096  # kMstatMaxGrid
THIN_DIMS = (70, 5, 9000)
THIN_ORIGIN = (1, 1, 1)
THIN_VOLUME_DIMS = (72, 7, 9002)


def thin_volume(layout):
    """u16: every code; f32: normal deviates."""
    k = ("thin", layout)
    if k not in _big:
        nx, ny, nz = THIN_VOLUME_DIMS
        rng = np.random.default_rng(29)
        if layout == "u16":
            v = rng.integers(0, 65536, (nz, ny, nx)).astype(F)
        else:
            v = (rng.standard_normal((nz, ny, nx)) * 1000.0).astype(F)
        v.setflags(write=False)
        _big[k] = v
    return _big[k]


def thin_labels():
    """Five large labels, slabs of 2000 slices (a workgroup's successive tiles, 1024 slices apart, stay in
    one or change to the next), every 37th voxel a speck of label 9 (its place in the wave's 64 lanes
    moves from tile to tile, so a lane that kept a speck later heads a long run and the reverse), and 100
    unset slices."""
    nx, ny, nz = THIN_DIMS
    idx = np.arange(nx * ny * nz, dtype=np.uint32)
    z = idx // np.uint32(nx * ny)
    lab = np.uint32(1) + z // np.uint32(2000)
    lab[::37] = 9
    lab[(z >= 3000) & (z < 3100)] = 0
    return lab.reshape(nz, ny, nx)


def lane_events(lab, grid=MAX_GRID, step=16):
    """What the lanes of the label pass meet on `lab`, restated from the kernel's rule for every
    step-th workgroup: a lane that heads a run of a listed label either keeps it (`first`: it held
    nothing), adds it to the sums it keeps for the same label (`merge`), sends it on alone because what
    it keeps is larger (`flush_smaller`), or sends what it keeps on and keeps the run (`replace`)."""
    bz, by, bx = lab.shape
    tiles_x, tiles_y = -(-bx // 64), -(-by // 4)
    tiles = tiles_x * tiles_y * bz
    events = dict(first=0, merge=0, flush_smaller=0, replace=0, tiles=tiles, most_tiles_a_workgroup=-(-tiles // grid))
    for b in range(0, min(grid, tiles), step):
        kept = {}  # (wave, lane) -> [label, voxels]
        for t in range(b, tiles, grid):
            tx, r = t % tiles_x, t // tiles_x
            ty, k = r % tiles_y, r // tiles_y
            for w in range(4):
                j = ty * 4 + w
                if j >= by:
                    continue
                row = np.zeros(64, np.uint32)
                part = lab[k, j, tx * 64:tx * 64 + 64]
                row[:part.size] = part
                heads = np.flatnonzero(np.concatenate([[True], row[1:] != row[:-1]]))
                ends = np.concatenate([heads[1:], [64]])
                for h, e in zip(heads, ends):
                    if row[h] == 0:
                        continue
                    have = kept.get((w, int(h)))
                    n = int(e - h)
                    if have is None:
                        events["first"] += 1
                        kept[(w, int(h))] = [int(row[h]), n]
                    elif have[0] == row[h]:
                        events["merge"] += 1
                        have[1] += n
                    elif have[1] > n:
                        events["flush_smaller"] += 1
                    else:
                        events["replace"] += 1
                        kept[(w, int(h))] = [int(row[h]), n]
    return events


def table_of(labels):
    """A table of LABEL_COMPONENT_DTYPE records with the labels of `labels` (only .label is read)."""
    u = np.unique(labels[labels != 0])
    t = np.zeros(u.size, label_ref.COMPONENT_DTYPE)
    t["label"] = u
    t["voxels"] = 0x7777  # (never read)
    return t
