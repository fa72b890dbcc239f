"""The NumPy statement of include/vr/vr_mstat.h -- test helper.

A grid is a (bz, by, bx) array in box-linear order; `vol` below is the volume already cropped to the
grid (crop()), as float32: a voxel's value is f = (float)stored.

regions():     one record per table label, in table order: voxels, nan, the extremes over the
               non-NaN voxels with the smallest box-linear index that holds each, and the sums --
               exact integers on integer storage (int64 / uint64, converted to double once), and on
               f32 storage math.fsum of (double)f and of the exact products (double)f * (double)f.
mask_stats():  the one region (label 1) of the set voxels, and with hist the bins and the info of
               hist_ref.histogram over them.
window():      label_ref.in_window under the mask.
sum_bounds():  the header's bound on an f32 sum, from n and A alone.
"""
import math

import numpy as np

import hist_ref
import label_ref

F = np.float32
NONE = 0xFFFFFFFF
REGION_DTYPE = np.dtype([("label", "<u4"), ("reserved", "<u4"), ("voxels", "<u8"), ("nan", "<u8"),
                         ("vmin", "<f4"), ("vmax", "<f4"), ("min_index", "<u4"), ("max_index", "<u4"),
                         ("sum", "<f8"), ("sum2", "<f8"), ("reserved2", "<u8")])
assert REGION_DTYPE.itemsize == 64


def crop(vol, origin, shape):
    """The (bz, by, bx) = shape grid of vol whose voxel (0, 0, 0) is volume voxel origin = (x, y, z)."""
    x, y, z = origin
    bz, by, bx = shape
    v = np.asarray(vol)[z:z + bz, y:y + by, x:x + bx]
    assert v.shape == tuple(shape)
    return v.astype(F)


def empty_records(table_labels):
    out = np.zeros(len(table_labels), REGION_DTYPE)
    out["label"] = table_labels
    out["vmin"], out["vmax"] = np.inf, -np.inf
    out["min_index"] = out["max_index"] = NONE
    return out


def _fsum(d):
    """The correctly rounded sum of the doubles d; IEEE's result where an infinity is among them."""
    if not np.isfinite(d).all():
        with np.errstate(invalid="ignore"):
            return float(np.sum(d, dtype=np.float64))
    return math.fsum(d.tolist())


def regions(vol, labels, table_labels, int_storage):
    """(records in table order, info dict).  table_labels: ascending, non-zero."""
    v = np.asarray(vol, F).reshape(-1)
    lab = np.asarray(labels).reshape(-1)
    assert v.size == lab.size
    tab = np.asarray(table_labels, np.uint32)
    assert tab.size == 0 or (tab[0] != 0 and np.all(tab[1:] > tab[:-1]))
    out = empty_records(tab)
    sel = np.flatnonzero(lab)
    info = {"voxels": int(lab.size), "set": int(sel.size), "unlisted": int(sel.size), "regions": int(tab.size)}
    if not tab.size or not sel.size:
        return out, info
    pos = np.searchsorted(tab, lab[sel])
    listed = (pos < tab.size) & (tab[np.minimum(pos, tab.size - 1)] == lab[sel])
    info["unlisted"] = int(sel.size - listed.sum())
    sel, slot = sel[listed], pos[listed]
    if not sel.size:
        return out, info
    o = np.argsort(slot, kind="stable")  # (the indices stay ascending inside a region)
    sel, slot = sel[o], slot[o]
    uniq, starts, counts = np.unique(slot, return_index=True, return_counts=True)
    rep = np.repeat(np.arange(uniq.size), counts)
    f = v[sel]
    isn = np.isnan(f)
    out["voxels"][uniq] = counts
    out["nan"][uniq] = np.add.reduceat(isn.astype(np.int64), starts)
    vmin = np.minimum.reduceat(np.where(isn, F(np.inf), f), starts)
    vmax = np.maximum.reduceat(np.where(isn, F(-np.inf), f), starts)
    out["vmin"][uniq], out["vmax"][uniq] = vmin, vmax
    out["min_index"][uniq] = np.minimum.reduceat(np.where(~isn & (f == vmin[rep]), sel, NONE), starts)
    out["max_index"][uniq] = np.minimum.reduceat(np.where(~isn & (f == vmax[rep]), sel, NONE), starts)
    if int_storage:
        assert not isn.any() and np.all(f == np.rint(f)) and np.all(np.abs(f) <= 65535)
        iv = f.astype(np.int64)
        assert sel.size * 65535 ** 2 < 2 ** 63  # (the integer sums below cannot wrap)
        out["sum"][uniq] = np.add.reduceat(iv, starts).astype(np.float64)  # (int64 -> double: one rounding)
        out["sum2"][uniq] = np.add.reduceat(iv * iv, starts).astype(np.uint64).astype(np.float64)
    else:
        d = np.where(isn, 0.0, f.astype(np.float64)) + 0.0  # (a zero term is +0.0 whatever its sign: the header)
        s, s2 = d.copy()[starts], (d * d)[starts]  # a region of one voxel: the term itself
        for g in np.flatnonzero(counts > 1):
            part = d[starts[g]:starts[g] + counts[g]][~isn[starts[g]:starts[g] + counts[g]]]
            s[g], s2[g] = _fsum(part), _fsum(part * part)  # (the product of two f32 is exact in double)
        out["sum"][uniq], out["sum2"][uniq] = s, s2
    return out, info


def mask_stats(vol, mask, int_storage, hist=None):
    """(the record, bins or None, hist info or None) of the set voxels of `mask`; hist = (nbins, lo, hi)."""
    m = np.asarray(mask).reshape(-1) != 0
    rec, _ = regions(vol, m.astype(np.uint32), [1], int_storage)
    if hist is None:
        return rec[0], None, None
    nbins, lo, hi = hist
    bins, hinfo = hist_ref.histogram(np.asarray(vol, F).reshape(-1)[m], lo, hi, nbins)
    return rec[0], bins, hinfo


def window(vol, mask, lo, hi):
    """(out (bz, by, bx) uint8, info dict); mask None: every voxel is set."""
    v = np.asarray(vol, F)
    s = np.ones(v.shape, bool) if mask is None else np.asarray(mask).reshape(v.shape) != 0
    out = (s & label_ref.in_window(v, lo, hi)).astype(np.uint8)
    return out, {"voxels": int(v.size), "in_set": int(s.sum()), "out_set": int(out.sum())}


def sum_bounds(values):
    """((n - 1) * 2^-52 * A, the same for the squares) of the non-NaN f32 `values`: the header's
    bound on |sum - S| for every order of addition, from n and the sum of magnitudes alone."""
    f = np.asarray(values, F).reshape(-1)
    d = f[~np.isnan(f)].astype(np.float64)
    n = d.size
    if n < 2:
        return 0.0, 0.0
    return (n - 1) * 2.0 ** -52 * _fsum(np.abs(d)), (n - 1) * 2.0 ** -52 * _fsum(d * d)


def normalised(rec):
    """A copy of the record(s) with the sign of a zero extreme dropped (the header leaves it free)."""
    r = np.array(rec, REGION_DTYPE, copy=True)
    r["vmin"] = r["vmin"] + F(0.0)
    r["vmax"] = r["vmax"] + F(0.0)
    return r


def same_but_sums(got, want):
    """Every field but sum and sum2, byte for byte (zero extremes by value)."""
    a, b = normalised(got), normalised(want)
    a["sum"] = a["sum2"] = b["sum"] = b["sum2"] = 0.0
    return a.tobytes() == b.tobytes()


def same_records(got, want):
    return normalised(got).tobytes() == normalised(want).tobytes()
