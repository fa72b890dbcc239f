"""The reference of include/vr/vr_label.h in numpy -- test helper.

Connected components of a value window by hooking and pointer jumping on the neighbour-pair
lists: every pair of neighbouring in-voxels hangs the larger of its two current roots under the
smaller (the minimum over all pairs that name a root), then every parent is replaced by its
parent until nothing moves; rounds repeat until every pair has one root.  A root is then the
smallest box-linear index of its component, which is the header's label minus one.

Volumes are (nz, ny, nx) arrays, boxes ((x0, y0, z0), (x1, y1, z1)) half open, seeds (x, y, z):
the binding's conventions.
"""
from collections import deque

import numpy as np

F = np.float32
COMPONENT_DTYPE = np.dtype([("label", "<u4"), ("reserved", "<u4"), ("voxels", "<u8"),
                            ("bbox_min", "<u4", 3), ("bbox_max", "<u4", 3), ("sum", "<u8", 3)])

# the neighbour offsets (dx, dy, dz) that come before a voxel in (z, y, x) order
OFFSETS_6 = [(-1, 0, 0), (0, -1, 0), (0, 0, -1)]
OFFSETS_26 = [(dx, dy, dz) for dz in (-1, 0) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
              if (dz, dy, dx) < (0, 0, 0)]
assert len(OFFSETS_26) == 13 and set(OFFSETS_6) <= set(OFFSETS_26)


def offsets(connectivity):
    assert connectivity in (6, 26)
    return OFFSETS_6 if connectivity == 6 else OFFSETS_26


def crop(vol, box):
    v = np.asarray(vol)
    if box is None:
        return v, (0, 0, 0)
    (x0, y0, z0), (x1, y1, z1) = box
    return v[z0:z1, y0:y1, x0:x1], (x0, y0, z0)


def in_window(v, lo, hi):
    """lo <= f && f <= hi in f32: a NaN is never in, -0.0 compares as 0."""
    f = np.asarray(v).astype(F)
    with np.errstate(invalid="ignore"):
        return (f >= F(lo)) & (f <= F(hi))


def _pairs(inm, connectivity):
    nz, ny, nx = inm.shape
    idx = np.arange(inm.size, dtype=np.int64).reshape(inm.shape)
    A, B = [], []
    for dx, dy, dz in offsets(connectivity):
        def sl(d, n):  # (the voxel's slice, the neighbour's slice) along one axis
            return (slice(max(0, -d), n - max(0, d)), slice(max(0, d), n - max(0, -d)))
        (zs, zn), (ys, yn), (xs, xn) = sl(dz, nz), sl(dy, ny), sl(dx, nx)
        m = inm[zs, ys, xs] & inm[zn, yn, xn]
        A.append(idx[zs, ys, xs][m])
        B.append(idx[zn, yn, xn][m])
    return np.concatenate(A), np.concatenate(B)


def label_array(inm, connectivity):
    """uint32 labels of a boolean (bz, by, bx) array: 0, or 1 + the component's smallest index."""
    A, B = _pairs(inm, connectivity)
    parent = np.arange(inm.size, dtype=np.int64)
    while A.size:
        ra, rb = parent[A], parent[B]
        m = ra != rb
        if not m.any():
            break
        A, B, ra, rb = A[m], B[m], ra[m], rb[m]
        hi, lo = np.maximum(ra, rb), np.minimum(ra, rb)
        order = np.argsort(-lo, kind="stable")  # the smallest lo is assigned last and stays
        parent[hi[order]] = lo[order]
        while True:
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp
    return np.where(inm.reshape(-1), parent + 1, 0).astype(np.uint32).reshape(inm.shape)


def table(labels, origin=(0, 0, 0)):
    """(records sorted by label, info dict) of a label array whose voxel (0, 0, 0) is volume voxel
    `origin` (x, y, z)."""
    lab = labels.reshape(-1)
    sel = np.flatnonzero(lab)
    info = {"voxels": int(lab.size), "in_voxels": int(sel.size), "components": 0,
            "largest_voxels": 0, "largest_label": 0}
    if not sel.size:
        return np.zeros(0, COMPONENT_DTYPE), info
    roots, inv = np.unique(lab[sel], return_inverse=True)
    nz, ny, nx = labels.shape
    coords = [sel % nx + origin[0], (sel // nx) % ny + origin[1], sel // (nx * ny) + origin[2]]
    order = np.argsort(inv, kind="stable")
    starts = np.searchsorted(inv[order], np.arange(roots.size))
    rec = np.zeros(roots.size, COMPONENT_DTYPE)
    rec["label"] = roots
    rec["voxels"] = np.bincount(inv, minlength=roots.size)
    for a in range(3):
        c = coords[a][order]
        rec["bbox_min"][:, a] = np.minimum.reduceat(c, starts)
        rec["bbox_max"][:, a] = np.maximum.reduceat(c, starts) + 1
        rec["sum"][:, a] = np.add.reduceat(c.astype(np.uint64), starts)
    big = int(np.argmax(rec["voxels"]))  # (the first maximum: the smallest label)
    info.update(components=int(roots.size), largest_voxels=int(rec["voxels"][big]),
                largest_label=int(rec["label"][big]))
    return rec, info


def label(vol, lo, hi, connectivity=6, box=None):
    """(labels (bz, by, bx) uint32, records, info) as OffscreenPass.label returns them."""
    v, origin = crop(vol, box)
    labels = label_array(in_window(v, lo, hi), connectivity)
    rec, info = table(labels, origin)
    return labels, rec, info


def region_grow(vol, seed, lo, hi, connectivity=6, box=None, labelled=None):
    """(mask (bz, by, bx) uint8, record dict) of the component of volume voxel `seed` (x, y, z)."""
    labels, rec, _ = labelled if labelled is not None else label(vol, lo, hi, connectivity, box)
    origin = (0, 0, 0) if box is None else box[0]
    lab = int(labels[seed[2] - origin[2], seed[1] - origin[1], seed[0] - origin[0]])
    mask = (labels == lab).astype(np.uint8) if lab else np.zeros(labels.shape, np.uint8)
    comp = {"label": 0, "voxels": 0, "bbox_min": (0, 0, 0), "bbox_max": (0, 0, 0), "sum": (0, 0, 0)}
    if lab:
        r = rec[np.searchsorted(rec["label"], lab)]
        comp = {"label": int(r["label"]), "voxels": int(r["voxels"]),
                "bbox_min": tuple(int(x) for x in r["bbox_min"]),
                "bbox_max": tuple(int(x) for x in r["bbox_max"]), "sum": tuple(int(x) for x in r["sum"])}
    return mask, comp


def bfs_label(inm, connectivity):
    """The same labels by a plain breadth-first search (small arrays: the check of label_array)."""
    nz, ny, nx = inm.shape
    out = np.zeros(inm.shape, np.uint32)
    both = [(dx, dy, dz) for dx, dy, dz in offsets(connectivity)]
    both += [(-dx, -dy, -dz) for dx, dy, dz in both]
    for z, y, x in zip(*np.nonzero(inm)):  # (ascending box-linear order: the first voxel is the root)
        if out[z, y, x]:
            continue
        lab = 1 + x + nx * (y + ny * z)
        out[z, y, x] = lab
        q = deque([(x, y, z)])
        while q:
            cx, cy, cz = q.popleft()
            for dx, dy, dz in both:
                px, py, pz = cx + dx, cy + dy, cz + dz
                if 0 <= px < nx and 0 <= py < ny and 0 <= pz < nz and inm[pz, py, px] and not out[pz, py, px]:
                    out[pz, py, px] = lab
                    q.append((px, py, pz))
    return out


_cache = {}


def cached(key, make_volume, lo, hi, connectivity=6, box=None):
    """One reference per key for the whole test session (never modified by the tests)."""
    k = (key, float(lo), float(hi), int(connectivity), box)
    if k not in _cache:
        labels, rec, info = label(make_volume(), lo, hi, connectivity, box)
        labels.setflags(write=False)
        rec.setflags(write=False)
        _cache[k] = (labels, rec, info)
    return _cache[k]
