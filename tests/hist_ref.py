"""The NumPy statement of include/vr/vr_hist.h -- test helper.

edges():   e[b] = f32(lo + (b * (hi - lo)) / nbins), left to right in float64, rounded once.
histogram(): a voxel with lo <= v <= hi counts in the largest b with e[b] <= v
             (np.searchsorted(e, v, side="right") - 1); v < lo -> below, v > hi -> above,
             NaN -> nan; the extremes over the non-NaN voxels.  Volumes are indexed [z, y, x];
             a box is ((x0, y0, z0), (x1, y1, z1)), half open.
window():  the percentile window of vr_hist_window.
"""
import math

import numpy as np


def edges(lo, hi, nbins):
    lo, hi = np.float64(np.float32(lo)), np.float64(np.float32(hi))
    b = np.arange(nbins, dtype=np.float64)
    return (lo + (b * (hi - lo)) / np.float64(nbins)).astype(np.float32)


def histogram(vol, lo, hi, nbins, box=None):
    """(uint64 bins, info dict) of the float32 values of vol (or of its box)."""
    v = np.asarray(vol)
    if box is not None:
        (x0, y0, z0), (x1, y1, z1) = box
        v = v[z0:z1, y0:y1, x0:x1]
    v = v.astype(np.float32).ravel()
    lo, hi = np.float32(lo), np.float32(hi)
    e = edges(lo, hi, nbins)
    isnan = np.isnan(v)
    ok = v[~isnan]
    below = ok < lo
    above = ok > hi
    inside = ok[~below & ~above]
    b = np.searchsorted(e, inside, side="right") - 1
    assert b.size == 0 or (b.min() >= 0 and b.max() < nbins)
    bins = np.bincount(b, minlength=nbins).astype(np.uint64)
    info = {"voxels": int(v.size), "below": int(below.sum()), "above": int(above.sum()),
            "nan": int(isnan.sum()),
            "vmin": np.float32(ok.min()) if ok.size else np.float32(np.inf),
            "vmax": np.float32(ok.max()) if ok.size else np.float32(-np.inf)}
    assert int(bins.sum()) + info["below"] + info["above"] + info["nan"] == info["voxels"]
    return bins, info


def window(bins, lo, hi, p_lo, p_hi):
    """(vmin, vmax) as float32, or None for what vr_hist_window refuses."""
    bins = np.asarray(bins, dtype=np.uint64)
    nbins = bins.size
    lo, hi = np.float32(lo), np.float32(hi)
    if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi and 1 <= nbins <= 4096):
        return None
    if not (0.0 <= p_lo < p_hi <= 1.0):
        return None
    c = np.cumsum(bins, dtype=np.uint64)
    n = int(c[-1])
    if n == 0:
        return None
    t0 = int(math.floor(p_lo * float(n)))
    t1 = max(1, int(math.ceil(p_hi * float(n))))
    ci = [int(x) for x in c]
    b0 = next(b for b in range(nbins) if ci[b] > t0)
    b1 = next(b for b in range(nbins) if ci[b] >= t1)
    e = edges(lo, hi, nbins)
    return e[b0], (hi if b1 == nbins - 1 else e[b1 + 1])


def same_info(got, ref):
    """The info dicts agree: counts exactly, the extremes by == (the sign of a zero is free)."""
    return (all(int(got[k]) == int(ref[k]) for k in ("voxels", "below", "above", "nan"))
            and np.float32(got["vmin"]) == np.float32(ref["vmin"])
            and np.float32(got["vmax"]) == np.float32(ref["vmax"]))


def edge_values(lo, hi, nbins):
    """Every edge, its f32 predecessor, hi and hi's successor: 2 nbins + 2 values, of which each
    bin holds exactly 2 (its own edge and the next edge's predecessor; the last bin its edge and
    hi), one lies below (lo's predecessor) and one above (hi's successor) -- provided the edges
    are distinct, which the caller's (lo, hi, nbins) must ensure."""
    e = edges(lo, hi, nbins)
    hi = np.float32(hi)
    v = np.concatenate([e, np.nextafter(e, np.float32(-np.inf)), [hi],
                        [np.nextafter(hi, np.float32(np.inf))]]).astype(np.float32)
    return v
